/*
 * unet_hip.h — C ABI of libunet_hip.so: the MI355X (gfx950) U-Net forward+backward hot path.
 *
 * Drop-in boundary for nsirons/DL-unet's `Unet.forward` (+ its autograd backward) and the
 * step either side of it.  Each entry point names the reference interface it replaces
 * (file:line in the reference repo).  Plain C: pointers are DEVICE pointers unless stated,
 * sizes are ints/size_t, `stream` is a hipStream_t passed as void* (0 = default stream).
 *
 * Conventions
 *   - return 0 = ok; <0 = library error (UNET_E_*); >0 = hipError_t.  unet_last_error()
 *     returns a thread-local message.  No entry point synchronises the host or allocates
 *     device memory, except unet_create()/unet_destroy() (a 4 KiB zero page per handle).
 *   - Public tensors keep the reference's layouts: images/logits NCHW fp32, conv weights
 *     OIHW, transposed-conv weights IOHW, int64 labels/masks.  Internally activations are
 *     NHWC fp32 (per-op entry points take NHWC).
 *   - The caller owns every buffer, including the workspace (size: unet_workspace_bytes).
 *   - All work is enqueued on the caller's stream; a handle is re-entrant per stream: what a forward plans (workspace
 *     layout, arithmetic mode) is kept with its plan for the backward.  Process-wide are only the switches: unet_set_math
 *     (the default of handles created with math = -1, and of the per-op entry points), unet_set_overlap, unet_set_lds_dma
 *     and unet_profile_*; set them while no call is in flight.
 *   - One process per GPU: a handle's calls must be made while its device is the current HIP device (checked).
 */
#ifndef UNET_HIP_H
#define UNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UNET_N_PARAMS 46          /* 23 layers x (weight, bias), network.py:23-58 order */
#define UNET_N_LAYERS 23
#define UNET_MAX_CLASSES 16        /* unet_create_classes: 2 <= n_classes <= 16 */

enum {
    UNET_E_BADSIZE  = -1,         /* S must be 16L+60 with L even >= 8 (network.py:124-127, Q7) */
    UNET_E_BADARG   = -2,
    UNET_E_NOTREADY = -3,         /* backward without a training forward on this workspace: this handle has no plan at that
                                     address (see "plans a handle keeps" at unet_backward); nothing is enqueued or written */
    UNET_E_UNSUPPORTED = -4,
    UNET_E_COMM     = -5          /* RCCL error (data parallel) */
};

typedef struct unet_handle unet_handle;

typedef struct unet_config {
    int base_ch;                  /* 64 in the reference (network.py:23); 32 for config #5 */
    int device;                   /* HIP device ordinal */
    int math;                     /* arithmetic of this handle's forwards/backwards (codes below); -1 = follow unet_set_math */
} unet_config;

const char *unet_last_error(void);
int unet_abi_version(void);     /* 4.  (2: unet_config::math, unet_dp_*;  3: unet_bce_step, unet_set_grad_scale, unet_set_overlap;  4: unet_backward_input) */

/* Arithmetic of the dense contractions — the process default, used by the per-op entry points and by handles created
 * with math = -1 (read when a forward is planned; its backward keeps that forward's mode):
 * 3 = fp32 on the fp32 MFMA, the stride-1 3x3 layers' forward and dgrad as Winograd F(2x2,3x3) (default: 16 of the 36
 *     multiplies of the direct correlation, all arithmetic fp32, same parity tolerances as mode 0),
 * 0 = fp32 on the fp32 MFMA, direct correlation everywhere (fmaf-chain numerics),
 * 1 = bf16x3: fp32 operands split into two bf16 terms, three bf16 MFMAs per product, fp32 accumulation
 *     (~16-bit products; logits stay within ~1e-5 of fp32),
 * 2 = bf16 (BASELINE config #3): activations, their gradients and the packed filters are bf16 IN HBM (NHWC, 2 B/element;
 *     the workspace halves), every contraction runs on the bf16 matrix cores with fp32 accumulation; parameters, their
 *     gradients, biases, the input image, logits and dlogits stay fp32 (fp32 master weights).  In this mode the per-op
 *     entry points below take bf16 activation / activation-gradient tensors where they take fp32 in the other modes.
 * Also settable with UNET_MATH.                                                                                       */
int unet_set_math(int mode);
int unet_get_math(void);
/* Operand staging of the MFMA kernels: 1 (default) = LDS-DMA through buffer descriptors whenever every tensor of a launch is
 * below 2 GiB, else global_load_lds; 0 = always global_load_lds (what tensors >= 2 GiB take, e.g. config #5 at batch 16).
 * A tuning / test knob: results are bit-identical, with one exception - the fp32 up-conv weight and bias gradient (modes 0
 * and 3): at 1 it is the pixel-linear kernel (wgrad_up<f32>), at 0 the row-walking one (wgrad<2;2;2;split0>), which sums
 * the pixels in another order (same error bound, different rounding).  The bf16 kernels (mode 2) always stage by buffer
 * descriptor and ignore the knob; so does the bf16x3 implicit GEMM (mode 1).  Also settable with UNET_LDS_DMA.
 * (UNET_WGRAD_UP=0, an A/B switch read once per process, moves the fp32 up-conv weight gradient to the row-walking kernel
 *  in modes 0 and 3; it does not apply to mode 2, whose bf16 tensors have no row-walking kernel.)                 */
int unet_set_lds_dma(int mode);

/* ---- handle ------------------------------------------------------------------------------
 * replaces: Unet.__init__ bookkeeping that is not parameters (network.py:20-58).
 * unet_create makes the reference's 2-class net.  unet_create_classes makes a K-class one (Unet(n_classes=K), 2 <= K <= 16):
 * only the head changes - finalconv is [K,C,1,1] + [K] (parameter indices 44/45), logits and dlogits are [B,K,So,So];
 * K = 2 is exactly unet_create.  unet_n_classes returns a handle's K.                                  */
int unet_create(unet_handle **out, const unet_config *cfg);
int unet_create_classes(unet_handle **out, const unet_config *cfg, int n_classes);
int unet_n_classes(const unet_handle *h);
int unet_destroy(unet_handle *h);

/* Size contract of the valid-conv net (functions.py:121-146 input_size_compute):
 * returns 0 and writes out_size = S-184 when S = 16L+60, L even >= 8; UNET_E_BADSIZE else. */
int unet_output_size(int S, int *out_size);
int unet_param_count(const unet_handle *h, int idx, size_t *numel);   /* idx in [0,46) */

/* Bytes of caller-provided workspace for a batch of B tiles of S x S.
 * training=1 also reserves gradient/activation-gradient storage for unet_backward.        */
size_t unet_workspace_bytes(const unet_handle *h, int B, int S, int training);

/* ---- whole path ---------------------------------------------------------------------------
 * replaces: Unet.forward (network.py:129-192), called at trainer.py:58,100 and tester.py:27.
 *   params : host array of 46 device pointers, reference state-dict order/layout (fp32)
 *   x      : [B,1,S,S] fp32;  logits : [B,K,S-184,S-184] fp32 NCHW (K = unet_n_classes, 2 for unet_create)
 *   training=1 keeps the activation stash in `workspace` for unet_backward.               */
int unet_forward(unet_handle *h, const void *const *params, const void *x, void *logits,
                 int B, int S, void *workspace, size_t workspace_bytes, int training,
                 void *stream);

/* Training forward with drop-out at the end of the contracting path (Ronneberger et al. 2015, section 3.1: "Drop-out layers at
 * the end of the contracting path perform further implicit data augmentation"; the reference has none: network.py:150-156).
 * Two sites, as in the authors' network definition: site 0 = conv42c's output (after its ReLU, before the pool, so conv51c
 * and the skip both see the dropped tensor), site 1 = conv52c's output (before upconv4).  Inverted, in place:
 *   y = keep ? x * s : 0,  s = 1.0f / (1.0f - p) in fp32, one fp32 multiply per element (bf16 tensors: rounded to nearest even)
 *   keep = word (idx & 3) of Philox4x32-10(counter, key) >= (uint32) min(floor(p * 2^32), 2^32 - 1)
 *   idx = linear index into the NHWC tensor;  key = (seed lo, seed hi);
 *   counter = (g lo, g hi, step lo, (step hi & 0x7fffffff) | site << 31),  g = idx >> 2
 * Always a training forward (activations kept, the plan remembered with p: the backward of this workspace scales the two
 * sites' gradients by s; the drop itself is in the consumers' ReLU masks).  Stateless: the caller owns seed and step.
 * 0 <= p < 1; p == 0 is exactly the plain forward with training=1.  Same workspace as unet_workspace_bytes(h, B, S, 1). */
int unet_forward_dropout(unet_handle *h, const void *const *params, const void *x, void *logits,
                         int B, int S, void *workspace, size_t workspace_bytes, float p,
                         unsigned long long seed, unsigned long long step, void *stream);
/* The keep flags (1 / 0 bytes) of elements [first, first + n) of a site's tensor, as the forward above draws them. */
int unet_dropout_mask(unsigned long long seed, unsigned long long step, int site, size_t first, size_t n, float p,
                      void *keep_u8, void *stream);

/* replaces: the autograd backward of every op in Unet.forward, triggered by
 * loss.backward() at trainer.py:77.
 *   dlogits : [B,K,So,So] fp32 NCHW (contiguous)
 *   grads   : host array of 46 device pointers, same shapes/layouts as params; OVERWRITTEN
 * Stages let the caller overlap the gradient all-reduce with the rest of the backward:
 * stage s in [0, unet_backward_stages()) must be run in increasing order; after stage s
 * returns, every gradient tensor listed by unet_backward_stage_params(s) is final (in
 * stream order).  unet_backward == all stages.
 *
 * The plans a handle keeps.  A training forward (unet_forward with training=1, unet_forward_dropout) leaves its plan - shape,
 * arithmetic mode, drop-out probability, workspace layout - in the handle, keyed by the workspace ADDRESS it was given; the
 * backward entry points find it by that address and return UNET_E_NOTREADY when the handle has none there (no forward ran
 * on that address on THIS handle: plans are per handle, and an address inside a workspace is another address).
 *   - Pending: from the training forward until the last backward stage of that workspace has been enqueued once.  Any number
 *     of forwards may be pending on one handle at a time, of any mix of shapes, arithmetic modes and drop-out
 *     probabilities, and their backwards may run in any order; every pending forward needs a live workspace of its own, so
 *     device memory is what bounds them.  A pending plan is never dropped to make room for another.  The one hard bound is
 *     1024 pending plans per handle (about 1.5 KB each), against callers that abandon forwards without ever running their
 *     backward or reusing the address: past it the oldest pending plan is dropped.
 *   - Finished: after that.  The plan stays for unet_backward_input, and a backward may be REPEATED on the workspace with no
 *     forward in between: no stage reads a gradient buffer it has not rewritten, so the repeat returns the same bits
 *     (grad_scale and the knobs below unchanged).  The handle keeps the 16 most recently finished plans; older ones are
 *     dropped, and a backward on their address returns UNET_E_NOTREADY.
 *   - A forward on an address replaces the plan at that address.  An inference forward (training=0) leaves none: a backward
 *     on a workspace that an inference forward has overwritten returns UNET_E_NOTREADY.  The handle sees addresses only: an
 *     inference forward (or any other write) at a DIFFERENT address inside the same allocation is not detected, and the
 *     backward of the training forward it damaged computes garbage.
 *   - Read when the backward runs: unet_set_grad_scale, unet_set_lds_dma, unet_set_overlap (they may change between a forward
 *     and its backward).  Read when the forward is planned: the arithmetic mode (unet_config::math / unet_set_math); the
 *     backward of a forward keeps that forward's mode whatever the default is by then.
 * A workspace_bytes below what the forward's plan needs is UNET_E_BADARG.                       */
int unet_backward(unet_handle *h, const void *const *params, const void *dlogits,
                  void *const *grads, void *workspace, size_t workspace_bytes, void *stream);
/* Weight gradients of each backward stage on an auxiliary stream of the handle, next to the dgrad chain (they only share dz);
 * the streams re-join before unet_backward_stage returns control of `stream`'s order, so callers see no difference (results
 * are bit-identical).  Process-wide: -1 (default; also UNET_OVERLAP) = by what was measured: on with bf16 tensors (+3 % per
 * step) and in fp32 at batches of <= 4 tiles (+0.2 ... +1.2 %), off in fp32 at larger batches (-1 % at B = 8); 0 / 1 force it.  Never active while unet_profile_enable(1) records per-launch events
 * (two streams would interleave them); an event / wait failure fails the stage. */
int unet_set_overlap(int on);
int unet_backward_stages(void);
int unet_backward_stage(unet_handle *h, int stage, const void *const *params,
                        const void *dlogits, void *const *grads, void *workspace,
                        size_t workspace_bytes, void *stream);
/* replaces: the gradient autograd returns for the input image when a caller asks for it (t.requires_grad; the reference's
 * trainer / tester never do: trainer.py:58, tester.py:27 - conv11c's dgrad is the one backward op of network.py:131 they skip).
 *   dx : [B,1,S,S] fp32, OVERWRITTEN.  Call after the LAST backward stage of the same forward has been enqueued on `stream`. */
int unet_backward_input(unet_handle *h, const void *const *params, void *dx, void *workspace, size_t workspace_bytes, void *stream);
/* writes up to cap parameter indices completed by `stage`; returns how many */
int unet_backward_stage_params(int stage, int *idx, int cap);

/* Algorithmic FLOPs (2*MAC) of one forward / forward+backward for B tiles of S. */
double unet_flops(const unet_handle *h, int B, int S, int backward);

/* Element size of the workspace's activation tensors for this handle's arithmetic: 2 (bf16, mode 2) or 4 (fp32). */
int unet_activation_bytes(const unet_handle *h);

/* Debug/introspection: byte offset into the workspace, extent e and channel count of a named NHWC
 * [B,e,e,C] buffer of the plan for (B,S,training): activations "a1_l","a2_l" (l=0..4), "t_l","u_l",
 * "d1_l","d2_l" (l=0..3); with training=1 also their gradients "g_*", "g_ts_l" and "xin". */
int unet_debug_buffer(const unet_handle *h, int B, int S, int training, const char *name,
                      size_t *offset, int *extent, int *channels);

/* ---- data parallel (the reference is single-device, main_main.py:157-158) -------------------------
 * Batch-sharded replicas, one process per GPU; the only exchange is the gradient all-reduce, done by RCCL over xGMI on
 * a communicator stream owned by the handle.  Rendezvous: rank 0 calls unet_dp_unique_id and the HOST carries the
 * UNET_DP_ID_BYTES to every rank (any channel), then every rank calls unet_dp_init.
 *   unet_dp_allreduce : in-place SUM all-reduce of `count` fp32 at `buf`, ordered after everything enqueued on `stream`
 *                       so far, running on the communicator stream (the caller's stream is not blocked: issue it after
 *                       each unet_backward_stage to overlap the bucket with the next stage)
 *   unet_dp_join      : `stream` waits for every collective issued so far (call before the optimizer step)
 *   unet_dp_broadcast : `count` fp32 from `root` to all ranks (initial parameters); same ordering as allreduce
 * Gradients are linear in dlogits, so SUM-reducing the gradients of dlogits / world gives the global-batch mean:
 *   unet_set_grad_scale : the backward of this handle reads dlogits * scale (applied inside the head's backward kernel, no
 *                         extra pass); 1.0 at creation.  A replica of a world-N job sets 1/N once. */
#define UNET_DP_ID_BYTES 128
int unet_set_grad_scale(unet_handle *h, float scale);
int unet_dp_unique_id(void *id_out_host);
int unet_dp_init(unet_handle *h, int rank, int world, const void *id_host);
int unet_dp_destroy(unet_handle *h);
int unet_dp_world(unet_handle *h);                /* ranks of the handle's communicator, 0 if none */
int unet_dp_rccl_version(void);                   /* ncclGetVersion of the bound librccl, 0 if it cannot be loaded */
int unet_dp_allreduce(unet_handle *h, void *buf, size_t count, void *stream);
int unet_dp_broadcast(unet_handle *h, void *buf, size_t count, int root, void *stream);
int unet_dp_join(unet_handle *h, void *stream);

/* ---- measurement -----------------------------------------------------------------------------
 * Optional HIP-event timing around kernel launches, recorded on the launch stream.  A pair of events per launch costs ~1 ms
 * per training step when every launch carries one, so bench.py selects only the dominant kernel kind inside its timed region
 * (unet_profile_select) and builds the per-layer table in a separate, fully instrumented pass.  Every launch records its kernel kind, the SURVEY 8a
 * row it belongs to, its algorithmic FLOPs (2*MAC, in-bounds taps only), the FLOPs the matrix cores execute for it
 * (Winograd: 16/36 of the direct count; tile padding included) and its algorithmic HBM bytes.
 * kind: 0 implicit GEMM (igemm*.hip), 1 weight gradient, 2 its split-K reduce, 3 Winograd 3x3 (wino.hip),
 *       4 conv11c stencil, 5 element-wise / reductions (pool, head, loss, SGD, packers), 6 RCCL collectives.
 * unet_profile_read synchronises on the recorded events and returns totals of one kind since the last reset.       */
int unet_profile_enable(int on);
/* launch kinds that get events while profiling is on: bit k = kind k (default: all) */
int unet_profile_select(unsigned kinds);
int unet_profile_reset(void);
int unet_profile_read(int kind, double *ms_total, long *launches, double *flops_total, double *exec_flops_total,
                      double *bytes_total);
/* one CSV line per recorded launch: kind,ms,gflop,exec_gflop,mbytes,row,tag */
int unet_profile_dump(const char *path);

/* ---- step-side kernels (L1-L3) -------------------------------------------------------------
 * L1 replaces nn.BCEWithLogitsLoss(weight=w)(preds, ll) + its backward (trainer.py:63-77).
 *   logits/target/dlogits : [B,2,H,W] fp32 contiguous; target is the one-hot `ll`
 *   weight : NULL, or fp32 with element strides (wsB,wsC,wsH,wsW) (0 = broadcast dim) —
 *            the caller decides the broadcast (reference: Q4 aligns B with the class axis)
 *   loss_out : 1 fp32 (mean over B*2*H*W); dlogits may be NULL; grad_scale multiplies the
 *            gradient (1/world_size for data parallel).  scratch: >= unet_bce_scratch_bytes */
size_t unet_bce_scratch_bytes(size_t numel);
int unet_bce_logits(const void *logits, const void *target, const void *weight,
                    long wsB, long wsC, long wsH, long wsW, int B, int H, int W,
                    void *loss_out, void *dlogits, float grad_scale, void *scratch, void *stream);
/* L1 + L2 of a training step in one pass (trainer.py:60-82): logits [B,2,H,W] fp32 addressed through element strides
 * (batch, class plane, row; unit pixel stride - the trainer's centre crop of preds is such a view), int64 labels [B,1,H,W]
 * in {0,1} instead of the one-hot target [1-y, y], the optional weight as in unet_bce_logits.  Writes the mean loss, the
 * dense dlogits [B,2,H,W] (x grad_scale; may be NULL) and the argmax mask [B,H,W] int64, ties -> class 0 (may be NULL).
 * scratch: >= unet_bce_step_scratch_bytes(B*H*W). */
size_t unet_bce_step_scratch_bytes(size_t npix);
int unet_bce_step(const void *logits, long xsB, long xsC, long xsH, const void *labels_i64, const void *weight,
                  long wsB, long wsC, long wsH, long wsW, int B, int H, int W, void *loss_out, void *dlogits,
                  float grad_scale, void *mask_i64, void *scratch, void *stream);
/* builds ll from integer labels on device: ll[:,0]=1-y, ll[:,1]=y (trainer.py:63-66) */
int unet_onehot2(const void *labels_i64, void *target, int B, int H, int W, void *stream);
/* L1 + L2 for K classes, the paper's loss (Ronneberger et al. 2015, eq. 1: a pixel-wise soft-max with a weighted cross-entropy):
 *   logits [B,K,H,W] fp32 through element strides (batch, class plane, row; unit pixel stride), 2 <= K <= 16;
 *   labels int64 [B,H,W] (dense) in [0, K); weight: NULL or a PER-PIXEL fp32 map through strides (wsB, wsH, wsW), 0 = broadcast.
 *   loss_out : 1 fp32 = mean over the B*H*W pixels of w * (logsumexp(l) - l_label) (max-subtracted; partials in double, fixed order)
 *   dlogits  : NULL or dense [B,K,H,W] = w * (softmax(l) - onehot(label)) / (B*H*W) * grad_scale
 *   mask_i64 : NULL or [B,H,W] argmax, ties -> the lowest class index (torch.argmax)
 *   invalid_u64 : NULL or 1 u64 = pixels whose label is outside [0, K): they are never used as an index and add no loss and no gradient.
 * scratch: >= unet_softmax_ce_scratch_bytes(B*H*W). */
size_t unet_softmax_ce_scratch_bytes(size_t npix);
int unet_softmax_ce_step(const void *logits, long xsB, long xsC, long xsH, int K, const void *labels_i64, const void *weight,
                         long wsB, long wsH, long wsW, int B, int H, int W, void *loss_out, void *dlogits, float grad_scale,
                         void *mask_i64, void *invalid_u64, void *scratch, void *stream);
/* L1 + L2 with an overlap loss: the soft Dice loss (Milletari et al. 2016) over the K-class soft-max, alone or added to the
 * cross-entropy above (nnU-Net's CE + Dice).  Logits, labels, weight, mask_i64, invalid_u64 and grad_scale as in
 * unet_softmax_ce_step; the weight map multiplies the CE term only.  With p = softmax(l) and v = the pixels whose label is in [0, K):
 *   I[b,k] = sum_v p_k [y = k]   P[b,k] = sum_v p_k   Y[b,k] = sum_v [y = k]   dice[b,k] = (2 I + s) / (P + Y + s),  s = smooth > 0
 *   L_dice = 1 - mean of dice over the counted (b,k);   L = ce_weight * L_ce + dice_weight * L_dice   (both weights >= 0, not both 0)
 *   flags    : UNET_DICE_BATCH sums I, P, Y over the batch before the ratio (one term per class); UNET_DICE_SKIP_BACKGROUND
 *              leaves class 0 out of the mean
 *   loss_out : 3 fp32 = L, L_ce, L_dice (partials in double, fixed order: bit-identical on every run and stream)
 *   dice_out : NULL or [B,K] fp32 ([1,K] with UNET_DICE_BATCH) = dice, of every class, counted or not
 *   dlogits  : NULL or dense [B,K,H,W] = grad_scale * (ce_weight * dL_ce/dl + dice_weight * dL_dice/dl),
 *              dL_dice/dl_j = p_j (g_j - sum_k g_k p_k), g_k = -(2 [y = k] / D - (2 I + s) / D^2) / terms at valid pixels, D = P + Y + s;
 *              0 on every plane of a pixel whose label is outside [0, K)
 * Three launches (sums, finish, gradient; the last only with dlogits), no host sync.  B <= 65535.
 * scratch: >= unet_dice_scratch_bytes(B, K, H, W) (0 for an empty shape). */
#define UNET_DICE_BATCH 1
#define UNET_DICE_SKIP_BACKGROUND 2
size_t unet_dice_scratch_bytes(int B, int K, int H, int W);
int unet_dice_step(const void *logits, long xsB, long xsC, long xsH, int K, const void *labels_i64, const void *weight,
                   long wsB, long wsH, long wsW, int B, int H, int W, float ce_weight, float dice_weight, float smooth, int flags,
                   void *loss_out, void *dice_out, void *dlogits, float grad_scale, void *mask_i64, void *invalid_u64,
                   void *scratch, void *stream);

/* L2 replaces preds.argmax(dim=1) (trainer.py:82, tester.py:30): [B,2,H,W] fp32 with row
 * stride ld (elements) and plane stride ps -> [B,H,W] int64; ties -> class 0.               */
int unet_argmax2(const void *logits, long batch_stride, long plane_stride, long row_stride,
                 void *out_i64, int B, int H, int W, void *stream);
/* K-way argmax (2 <= K <= 16) of [B,K,H,W] fp32 with the same strides -> [B,H,W] int64; ties -> the lowest class index. */
int unet_argmaxk(const void *logits, long batch_stride, long plane_stride, long row_stride, int K, void *out_i64, int B, int H, int W,
                 void *stream);

/* L3 replaces optim.SGD(lr, momentum).step() (trainer.py:30,78): for each of n tensors
 * buf = first ? g : mu*buf + g ; p -= lr*buf.  Pointer tables are HOST arrays.             */
int unet_sgd_momentum(void *const *params, const void *const *grads, void *const *bufs,
                      const size_t *numel, int n, float lr, float mu, int first_step,
                      void *stream);

/* L3 with an adaptive update (adam.hip): Adam (decoupled = 0, L2 decay) and AdamW (decoupled = 1) over n <= UNET_N_PARAMS fp32
 * tensors, torch.optim.Adam / AdamW without amsgrad and maximize.  Pointer tables and numel are HOST arrays; step >= 1 counts
 * this update, eps > 0, 0 <= beta < 1.  Per element, every operation rounded once to fp32, in this order:
 *    1  g = g * c                        only if grad_scale_dev != NULL: c = the one device float it points to
 *    2  g = g + wd * p                   decoupled = 0 and wd != 0
 *       p = p * decay                    decoupled = 1 and wd != 0;  decay = 1 - lr wd
 *    3  m = m + om1 * (g - m)            om1 = 1 - beta1
 *    4  v = beta2 * v + om2 * (g * g)    om2 = 1 - beta2
 *    5  d = sqrt(v) * rbc2 + eps         rbc2 = 1 / sqrt(1 - beta2^step)
 *    6  p = p - step_size * (m / d)      step_size = lr / (1 - beta1^step)
 * om1, om2, decay, rbc2 and step_size are formed on the host in double from the fp32 arguments and rounded to fp32 once each.
 * With step == 1, m and v count as 0 and exp_avg / exp_avg_sq are written, never read (as unet_sgd_momentum's first_step).
 * Subnormals are kept; sqrt and the division are correctly rounded.  The gradients are not written.  16 B read and 12 B
 * written per element (8 B read at step 1).  Non-finite values propagate as IEEE has them. */
int unet_adam_step(void *const *params, const void *const *grads, void *const *exp_avg, void *const *exp_avg_sq,
                   const size_t *numel, int n, float lr, float beta1, float beta2, float eps, float weight_decay,
                   int decoupled, long step, const void *grad_scale_dev, void *stream);
/* The global gradient norm and torch.nn.utils.clip_grad_norm_'s coefficient, without a host sync and without float atomics.
 *   unet_grad_sumsq_partials : host only: the number of 4096-element chunks of the n tensors (each tensor's last one may be
 *                      short; a zero-size tensor has none) = the fp64 partials unet_grad_sumsq writes for them.
 *   unet_grad_sumsq  : partials[partial_offset + c] = the sum of g^2 over chunk c of the call (fp64; exact squares, a fixed
 *                      order per lane, then wave, then block).  Several calls at increasing offsets cover more than
 *                      UNET_N_PARAMS tensors.
 *   unet_grad_norm_finish : one workgroup adds the n_partials partials in a fixed order in fp64 and writes two fp32:
 *                      out2[0] = (float)sqrt(sum), out2[1] = min(1, max_norm / (out2[0] + 1e-6)) in fp32; max_norm > 0.
 *                      A NaN norm gives a NaN coefficient, an infinite one 0.
 *   unet_grads_scale : g = g * c in place, c = the device float at scale_dev (for updates that do not take it themselves). */
size_t unet_grad_sumsq_partials(const size_t *numel, int n);
int unet_grad_sumsq(const void *const *grads, const size_t *numel, int n, void *partials, size_t partial_offset, void *stream);
int unet_grad_norm_finish(const void *partials, size_t n_partials, float max_norm, void *out2, void *stream);
int unet_grads_scale(void *const *grads, const size_t *numel, int n, const void *scale_dev, void *stream);

/* ---- callers either side of the path; fp32 images [B,H,W], int64 labels ----------
 * N2 overlap-tile front end, replaces mirror_transform + the [0,1] normalisation (data.py:184-188,
 * :249-277): out[b,0,Y,X] = x[b, r(Y), r(X)] with the reference's asymmetric reflection (top/left band
 * without the edge pixel, bottom/right band with it); minmax (from unet_minmax, [B][2]) may be NULL.   */
int unet_minmax(const void *x, int B, size_t n_per_image, void *out_minmax, void *stream);
int unet_mirror_pad(const void *x, int B, int n, int S, const void *minmax, void *out, void *stream);
/* N2 overlap-tile segmentation of images of any size (tester.segment; the reference crops test images to a square instead,
 * data.py:174-181): the ny x nx grid of So = S-184 output tiles is centred on the image, origin (oy0, ox0) <= 0
 * (tester.tile_grid); tile t = (b*ny + i)*nx + j reads rows [oy0 + i*So - 92, +S) and columns [ox0 + j*So - 92, +S) and
 * covers output rows [oy0 + i*So, +So), columns [ox0 + j*So, +So), clipped to the image.
 *   unet_tile_gather : img fp32 [B,H,W] (H, W >= 2) -> tiles_out fp32 [nt,1,S,S] = tiles t0 .. t0+nt-1, coordinates outside
 *                      the image mapped by numpy.pad(mode='reflect') (edge pixel not repeated, period 2(n-1) when the pad is
 *                      wider than the image; NOT unet_mirror_pad's asymmetric map); minmax ([B][2], from unet_minmax) may
 *                      be NULL, else each value becomes (x - min) / (max - min) (fp32, true division).
 *   unet_tile_stitch : logits fp32 [nt,2,So,So] of tiles t0 .. t0+nt-1 -> mask_i64 [B,H,W] = argmax (ties -> class 0, as
 *                      unet_argmax2) and, if prob_f32 is not NULL, prob_f32 [B,H,W] = 1 / (1 + exp(l0 - l1)), for every
 *                      pixel of those tiles inside the image; nothing else is written (each pixel has exactly one tile). */
int unet_tile_gather(const void *img, int B, int H, int W, const void *minmax, int S, int oy0, int ox0, int ny, int nx, long t0, int nt,
                     void *tiles_out, void *stream);
int unet_tile_stitch(const void *logits, int So, int oy0, int ox0, int ny, int nx, long t0, int nt, int B, int H, int W, void *mask_i64,
                     void *prob_f32, void *stream);
/*   unet_tile_stitch_k : the same grid contract for K classes (2 <= K <= 16): logits fp32 [nt,K,So,So] (16-byte aligned) ->
 *                      mask_i64 [B,H,W] = argmax, ties -> the lowest class, and, if prob_f32 is not NULL, prob_f32 [B,K,H,W] =
 *                      the softmax of the K logits (max-subtracted).                                                       */
int unet_tile_stitch_k(const void *logits, int So, int K, int oy0, int ox0, int ny, int nx, long t0, int nt, int B, int H, int W,
                       void *mask_i64, void *prob_f32, void *stream);
/* The same two for one of the 8 dihedral views of the image (tester.apply_view / segment(views=...)), without materialising it.
 * View code v = 0..7: t = v & 1 (transpose), fy = (v >> 1) & 1, fx = (v >> 2) & 1; the view has shape (Hv, Wv) = t ? (W, H) : (H, W)
 * and its pixel (y, x) is image pixel t ? (x', y') : (y', x'), y' = fy ? Hv-1-y : y, x' = fx ? Wv-1-x : x.  H, W are always the
 * image's; (ny, nx, oy0, ox0) is tester.tile_grid(Hv, Wv, S) and t = (b*ny + i)*nx + j indexes the tiles of this one view.
 *   unet_tile_gather_view : tiles_out = what unet_tile_gather gives on the materialised contiguous view, bit for bit.
 *   unet_tile_stitch_view : logits fp32 [nt,K,So,So] (2 <= K <= 16; 16-byte aligned for K > 2) -> each tile pixel's class
 *                      probabilities by the expressions of unet_tile_stitch (K = 2: class 1 only, prob_f32 [B,H,W]) and
 *                      unet_tile_stitch_k (K > 2: prob_f32 [B,K,H,W]), landed at the image pixel the view pixel came from.
 *                      phase bit 0 (FIRST): prob = p, else prob += p.  phase bit 1 (LAST): then, for this launch's pixels,
 *                      prob = sum / (float)n_views and mask_i64 [B,H,W] = prob > 0.5f (K = 2) or the argmax of the sums, ties ->
 *                      the lowest class (K > 2).  mask_i64 may be NULL unless LAST is set.  A view's tiles partition the image
 *                      and a launch touches each of its pixels once, without atomics: the order of the sum is the stream
 *                      order of the launches.                                                                               */
int unet_tile_gather_view(const void *img, int B, int H, int W, const void *minmax, int S, int view, int oy0, int ox0, int ny, int nx,
                          long t0, int nt, void *tiles_out, void *stream);
int unet_tile_stitch_view(const void *logits, int So, int K, int view, int oy0, int ox0, int ny, int nx, long t0, int nt, int B, int H,
                          int W, int phase, int n_views, void *prob_f32, void *mask_i64, void *stream);
/* N2 back end, replaces pred[:, :, pad:pad+n, pad:pad+n].argmax(dim=1) + IoU / Pixel_error counting
 * (tester.py:29-42, functions.py:174-213): mask int64 [B,n,n]; with labels int64 [B,n,n]:
 * stats u64 [B][3] = {sum(pred&label), sum(pred|label), sum|pred-label|} (exact integer atomics).      */
int unet_eval_masks(const void *logits, long batch_stride, long plane_stride, long row_stride, int pad,
                    const void *labels_i64, void *mask_i64, int B, int n, void *stats_u64, void *stream);
/* The K-class counterpart (2 <= K <= 16), same crop rule: mask int64 [B,n,n] = argmax (ties -> the lowest class); with labels
 * int64 [B,n,n]: conf_u64 [B][K][K], conf[b][i][j] = pixels of image b with label i predicted j, and invalid_u64 [B] = pixels
 * whose label is outside [0, K) (in no bin).  Exact: per-block LDS histograms, one integer atomic per bin.  */
int unet_eval_confusion(const void *logits, long batch_stride, long plane_stride, long row_stride, int pad, int K,
                        const void *labels_i64, void *mask_i64, int B, int n, void *conf_u64, void *invalid_u64, void *stream);
/* N3, replaces functions.class_balance (functions.py:82-117) for {0,1} labels: w = 1 on cells,
 * count(1)/count(0) on background; counts_u64 [B] receives count(1) (caller checks the degenerate case). */
int unet_class_balance(const void *labels_i64, int B, int H, int W, void *weights, void *counts_u64, void *stream);
/* Border weight map, replaces functions.weighted_map (functions.py:7-78: torch.unique counts, cv.connectedComponents(connectivity=4),
 * one cv.distanceTransform(DIST_L2, 0) per component, sort, w0 * exp(-(d1+d2)^2 / (2 sig2))) for {0,1} labels
 * [B,H,W], int64 (labels_dtype 0) or float32 (1); H != W allowed.  weights f32 [B,H,W]: 1 on cells; on background
 * w_c + w_d with w_c = count(1)/count(0) in fp32, truncated for int64 labels (the reference stores it in
 * torch.empty_like(gt)), d1 / d2 the exact distances to the nearest / second-nearest distinct 4-connected component
 * (d2 = 0 when the image has one).  counts_u64 [B] receives count(1), n_objects_i32 [B] the component count (the
 * caller checks the one-class case).  scratch: unet_weighted_map_scratch_bytes(B, H, W); sig2 <= ~5000.        */
size_t unet_weighted_map_scratch_bytes(int B, int H, int W);
int unet_weighted_map(const void *labels, int labels_dtype, int B, int H, int W, float w0, float sig2, void *weights_f32,
                      void *counts_u64, void *n_objects_i32, void *scratch, void *stream);
/* Cell instances of a foreground mask, replaces cv.connectedComponents as the reference calls it to number objects
 * (functions.py:47 with connectivity=4, the rule used here; data.py:375 when it writes the man_seg instance images; touching
 * cells are carved apart beforehand by preprocess_gt, data.py:195-219): mask [B,H,W], int64 (dtype 0) or float32 (1),
 * foreground = value != 0; H != W allowed, down to 1 x 1.  labels_i32 [B,H,W]: 0 on background, else the number 1..n of the
 * pixel's 4-connected component, the components numbered in raster order of their first pixel (scipy.ndimage.label's and
 * OpenCV's numbering); n_objects_i32 [B] = n.  Exact, and the cost does not depend on n (label.hip).
 * scratch: unet_label_components_scratch_bytes(B, H, W), initialised by the call.                                        */
size_t unet_label_components_scratch_bytes(int B, int H, int W);
int unet_label_components(const void *mask, int dtype, int B, int H, int W, void *labels_i32, void *n_objects_i32, void *scratch,
                          void *stream);
/* The same numbering for either phase of a mask and either connectivity (label.hip; functions.label_cells(connectivity=8)):
 * mask [B,H,W] of dtype 0 = int64, 1 = float32, 2 = int32, 3 = uint8.  phase 1 labels the pixels with mask != 0, phase 0 those
 * with mask == 0; connectivity 4 (the cross) or 8 (the full 3 x 3 neighbourhood).  labels_i32 [B,H,W]: the number 1..n of the
 * pixel's component, the components numbered in raster order of their first pixel (scipy.ndimage.label with the matching
 * structure), 0 on the other phase; n_objects_i32 [B] = n.  For phase 1, connectivity 4 the outputs are those of
 * unet_label_components bit for bit.  Exact, the cost does not depend on n.  Limits as unet_label_components (H * W < 2^31,
 * H <= 65535, B <= 65535), H != W allowed, down to 1 x 1.  Another dtype, connectivity or phase, a NULL pointer and a size
 * over the limit return an error and write nothing.
 * scratch: unet_label_components_conn_scratch_bytes(B, H, W), initialised by the call.                                        */
size_t unet_label_components_conn_scratch_bytes(int B, int H, int W);
int unet_label_components_conn(const void *mask, int dtype, int B, int H, int W, int connectivity, int phase, void *labels_i32,
                               void *n_objects_i32, void *scratch, void *stream);
/* Cleaning a foreground mask between the argmax and the instance map (clean.hip; functions.clean_mask; scipy's
 * binary_fill_holes, skimage's remove_small_holes / remove_small_objects / clear_border): mask [B,H,W] of dtype 0 = int64,
 * 1 = float32, 2 = int32, 3 = uint8, foreground = value != 0.  connectivity 4 or 8 is the foreground's; the background takes
 * the dual one (8 or 4).  A hole is a component of the background without a pixel in the first or last row or column; its area
 * is its own pixel count (foreground islands inside it do not count).  With fill != 0 a hole is filled when max_hole_area is
 * -1 (no limit) or its area <= max_hole_area.  The cells are the components of the mask after filling: one with area <
 * min_area is dropped as small (min_area 0 and 1 drop nothing), and with drop_border != 0 one that is not small and has a
 * pixel in the first or last row or column is dropped too.
 *   action_u8 [B,H,W] (may be NULL): 0 background that stays, 1 foreground kept, 2 filled, 3 dropped as small, 4 dropped on
 *                     the border
 *   out [B,H,W], mask's dtype: the input value where the action is 1, 1 where it is 2, else 0
 *   info_i64 [B][7]: holes filled, pixels filled, cells dropped as small, their pixels, cells dropped on the border, their
 *                     pixels, cells kept
 * A fixed list of launches on the stream for given arguments, no read-back; exact integers, the cost does not depend on the
 * number of holes or cells.  Limits as unet_label_components.  connectivity other than 4 or 8, max_hole_area < -1,
 * min_area < 0, another dtype, a NULL pointer (but action_u8) and a size over the limit return an error and write nothing.
 * scratch: unet_clean_mask_scratch_bytes(B, H, W) (13 bytes per pixel), initialised by the call.                             */
size_t unet_clean_mask_scratch_bytes(int B, int H, int W);
int unet_clean_mask(const void *mask, int dtype, int B, int H, int W, int connectivity, int fill, long long max_hole_area,
                    long long min_area, int drop_border, void *out, void *action_u8, void *info_i64, void *scratch, void *stream);
/* One row of exact integers per cell of an instance map, and of an image under it (measure.hip; functions.cell_sums; what
 * scipy.ndimage's sum_labels, find_objects, center_of_mass, minimum and maximum give one quantity at a time).  labels [B,H,W] of
 * label_dtype 0 = int64 or 2 = int32, 0 = background, ids anywhere in [0, n_max], n_max < 2^24, not necessarily consecutive or
 * connected.  image: NULL, or [B,H,W] of image_dtype 0 = int64, 2 = int32, 3 = uint8 with values in [0, 65536), or 1 = float32
 * with finite values.  Row i of image b (row 0 = the background, treated like any other id), over the pixels (y, x) with id i:
 *   area_i64    [B][n_max+1]    : pixels
 *   bbox_i32    [B][n_max+1][4] : y0, x0, y1, x1, half-open like scipy.ndimage.find_objects
 *   moments_i64 [B][n_max+1][5] : sum y, sum x, sum y^2, sum x^2, sum x y
 *   edges_i64   [B][n_max+1][3] : over the four sides of every pixel: frame (the side lies on the image frame), open (the
 *                                 neighbour has id 0 and i != 0), contact (the neighbour has another id; for i = 0 any non-zero
 *                                 id).  An edge between two ids counts once for each; the three sum to the crack-length perimeter
 *   vsum_64     [B][n_max+1][2] : sum v, sum v^2: int64 and exact for an integer image, fp64 for a float32 one (v^2 exact, the
 *                                 sums rounded per add; a run of equal ids in a row is summed in fixed order, the runs in arrival
 *                                 order).  May be NULL without an image and is not written then
 *   vrange_32   [B][n_max+1][2] : min v, max v, exact: int32, or float32 for a float32 image.  As vsum_64
 *   present_u8  [B][n_max+1]    : area > 0.  Every field of an absent id is 0
 *   status_u64  [B][2]          : pixels whose id is outside [0, n_max] (they index nothing and count nowhere else), pixels whose
 *                                 image value is refused (they add nothing to vsum and vrange)
 * Two memsets and two launches on the stream, no read-back; every integer is the same in every run; the cost does not depend on
 * the number of cells.  Limits: H, W <= 32768, B <= 65535: every sum fits 64 bits.  Another dtype, a NULL pointer, an image without vsum_64
 * and vrange_32, and a size over the limit return an error and write nothing.
 * scratch: unet_cell_sums_scratch_bytes(B, n_max) (128 bytes per row), initialised by the call.                              */
size_t unet_cell_sums_scratch_bytes(int B, int n_max);
int unet_cell_sums(const void *labels, int label_dtype, const void *image, int image_dtype, int B, int H, int W, int n_max, void *area_i64,
                   void *bbox_i32, void *moments_i64, void *edges_i64, void *vsum_64, void *vrange_32, void *present_u8, void *status_u64,
                   void *scratch, void *stream);
/* out_i32 [B,H,W] = map_i32[b * map_stride + labels[b,y,x]] (measure.hip; functions.select_cells): labels as above, map_stride 0
 * (one map [n_max+1] for the batch) or >= n_max + 1.  A pixel whose id is outside [0, n_max] becomes 0 and is counted in
 * status_u64 [B].  Limits and errors as above.                                                                               */
int unet_remap_labels(const void *labels, int label_dtype, int B, int H, int W, const void *map_i32, int n_max, long long map_stride,
                      void *out_i32, void *status_u64, void *stream);
/* The convex hull of every cell of an instance map, and the exact integers measured on it (hull.hip; functions.cell_hulls,
 * functions.hull_props; the definition in full: DESIGN.md section 4u; what a loop over cells with scipy.spatial.ConvexHull gives).
 * A pixel (y, x) is the closed unit square [x, x+1] x [y, y+1]; the hull of id i >= 1 of image b is the convex hull of the union
 * of its pixels' squares, i.e. of their integer corner points.  Ids need not be connected; id 0 is skipped.  labels, label_dtype,
 * n_max as unet_cell_sums; bbox_i32 [B][n_max+1][4] is unet_cell_sums's.  Row r = b (n_max + 1) + i has y1 - y0 + 1 levels if
 * i >= 1 and the id is present, else 0; level_offset_i64 [B (n_max+1) + 1] is the exclusive prefix sum of those counts and
 * n_levels = L their total.
 *   n_vertices_i32 [B][n_max+1]    : k, the vertices of the hull (collinear points dropped; >= 4 for a present id)
 *   area2_i64      [B][n_max+1]    : twice the area of the hull (shoelace sum)
 *   feret_max2_i64 [B][n_max+1]    : the largest squared distance between two vertices
 *   width_i64      [B][n_max+1][2] : (c, l2) of the hull edge (p, q) with the smallest c^2 / l2, the smaller l2 on equal ratios,
 *                                    where c = max over the vertices v of |cross(q - p, v - p)| and l2 = |q - p|^2: the minimum
 *                                    Feret diameter is c / sqrt(l2).  Compared in 128-bit integers, no division
 *   vertices_i32   [2 L][2]        : (x, y) in corner coordinates; row r owns [2 off[r], 2 off[r+1]): its k vertices, the left
 *                                    chain from (lo_0, y0) down to (lo_h, y1), then the right chain from (hi_h, y1) up to
 *                                    (hi_0, y0); the rest of the slice is 0
 *   status_u64     [B][2]          : pixels whose id is outside [0, n_max]; pixels outside the box given for their id, or whose
 *                                    id's level count does not fit its box or the tables.  Neither kind writes anything
 * Every output of row 0, of an absent id and of a row with an inconsistent box or level count is 0.  n_levels = 0 is legal:
 * vertices_i32 and scratch may be NULL then.  Three memsets and two launches on the stream, no read-back; every output is the same
 * in every run.  Limits as unet_cell_sums; another dtype, a NULL pointer, n_levels < 0 and a size over the limit return an error
 * and write nothing.
 * scratch: unet_cell_hulls_scratch_bytes(n_levels) (8 bytes per level: two 32-bit tables), initialised by the call.           */
size_t unet_cell_hulls_scratch_bytes(long long n_levels);
int unet_cell_hulls(const void *labels, int label_dtype, int B, int H, int W, int n_max, const void *bbox_i32, const void *level_offset_i64,
                    long long n_levels, void *n_vertices_i32, void *area2_i64, void *feret_max2_i64, void *width_i64, void *vertices_i32,
                    void *status_u64, void *scratch, void *stream);
/* Boundary scores: where the contour of a predicted mask lies against the contour of the ground truth (boundary.hip;
 * functions.mask_boundary, functions.surface_sums, functions.scores_from_surface, functions.boundary_scores).
 * The device gives exact integers and one fp64 sum per image and direction; the Hausdorff distance, its percentile, the average
 * symmetric surface distance and the normalised surface Dice are formed from them on the host.
 *   Region    mask != 0; with select = k >= 0 it is mask == k (the class-k region of a K-class label map; a float32 mask is compared
 *             with (float)k).  select = -1 means none.  Masks [B,H,W] of dtype 0 = int64, 1 = float32, 2 = int32, 3 = uint8.
 *   Contour   dA = the pixels of A that have a neighbour outside A: the 4-neighbours with connectivity 4, all eight with 8.
 *   Edge      edge 1 ("background", what scipy.ndimage.binary_erosion(border_value=0) and MONAI's get_mask_edges do): a pixel
 *             past the image is outside A, so region pixels on the frame are contour.  edge 0 ("ignore"): pixels past the image
 *             are nothing.
 *   Distance  for p in dA, d2(p) = the exact squared Euclidean distance (int32) to the nearest pixel of dB; defined only when dB is
 *             not empty.
 * unet_mask_boundary: out_u8 [B,H,W] = 1 on the contour of the mask's region, 0 elsewhere.  One launch, no scratch.
 * unet_surface_sums: both directions, P -> G (dir 0: d2 of the pixels of dP to dG) and G -> P (dir 1), in one call that never
 * synchronises.  record [B][2 dir] of 10 64-bit words each:
 *   [0] int64 n       = |dA|, also when dB is empty
 *   [1] int64 max_d2  = the largest d2
 *   [2] int64 lo, [3] int64 hi, [4] int64 rem : with j = floor((n - 1) q_num / q_den) and rem = (n - 1) q_num mod q_den, the j-th and
 *                       the min(j + 1, n - 1)-th smallest d2 (0-based): sqrt(lo) + rem / q_den (sqrt(hi) - sqrt(lo)) is
 *                       numpy.percentile(d, 100 q_num / q_den, method='linear').  0 <= q_num <= q_den, 1 <= q_den < 2^20
 *   [5..8] int64 within[i] = the pixels with d2 <= t2_i32[i], i < n_t2 (0 <= n_t2 <= 4; t2_i32 is a host array, read during the
 *                       call, every entry >= 0); 0 for i >= n_t2
 *   [9] fp64 sum      = the sum of sqrt(d2)
 * If dA or dB is empty, every word but n is 0 (the fp64 sum +0.0) and the d2 plane of that direction is -1 everywhere: the caller
 * tells "both empty" from "one empty" by the two n.  d2_pg_i32, d2_gp_i32 [B,H,W] (each may be NULL): d2 on dP (dG), -1 elsewhere.
 * Exact order statistics by a radix select on the device (digits of 11, 10 and 10 bits); every count is an integer atomic or a
 * fixed-order reduce, the fp64 sum is reduced per workgroup in a fixed order, written to the workgroup's own slot and added in slot
 * order by one workgroup: every output is bit-identical in every run and on every stream.  One memset and 11 launches.
 * Limits as unet_distance_map: H, W <= 32767, H * W < 2^31, B <= 65535; H != W allowed, down to 1 x 1.  A NULL pointer, another
 * dtype, connectivity, edge, a select below -1, a bad percentile or tolerance and a size over the limit return an error and write
 * nothing.
 * scratch: unet_surface_sums_scratch_bytes(B, H, W) (17 bytes per pixel, 32 per 256 pixels of a row and direction, and 32 KiB of
 * histograms per image), initialised by the call.                                                                              */
int unet_mask_boundary(const void *mask, int mask_dtype, int select, int B, int H, int W, int connectivity, int edge, void *out_u8, void *stream);
size_t unet_surface_sums_scratch_bytes(int B, int H, int W);
int unet_surface_sums(const void *pred, int pred_dtype, int pred_select, const void *gt, int gt_dtype, int gt_select, int B, int H, int W,
                      int connectivity, int edge, long long q_num, long long q_den, const int *t2_i32, int n_t2, void *record,
                      void *d2_pg_i32, void *d2_gp_i32, void *scratch, void *stream);
/* The integers of the Cell Tracking Challenge SEG measure, the score behind the goals of trainer.py:20-26 (Ronneberger et al.
 * 2015, Table 2): gt_i32, pred_i32 id maps int32 [B,H,W], 0 = background, gt ids anywhere in [0, ng_max] (not necessarily
 * consecutive, an object not necessarily connected), pred ids in [0, np_max]; ng_max, np_max < 2^24.
 *   area_gt_u32 [B][ng_max+1], area_pred_u32 [B][np_max+1] : pixels per id (index 0 = background)
 *   match_i32 [B][ng_max+1] : for g >= 1 the p >= 1 with 2 |g n p| > area_gt[g] (strict, so at most one), else 0;  [b][0] = 0
 *   inter_u32 [B][ng_max+1] : that |g n p|, else 0
 *   status_u64 [B][2]       : {pixels whose gt or pred id is outside its range (negative included): used as no index and
 *                              counted nowhere else;  pixels dropped because the pair table was full: if non-zero, match and
 *                              inter of that image are invalid and the caller repeats the call with a larger table}
 * table_slots: a power of two, the slots of the open-addressing table of distinct (b, g, p) pairs with g, p >= 1, shared by
 * the batch; a table with more slots than B*H*W cannot fill up.  Exact integer atomics: results are the same in every run.
 * scratch: unet_instance_overlap_scratch_bytes(B, ng_max, np_max, table_slots), initialised by the call.                 */
size_t unet_instance_overlap_scratch_bytes(int B, int ng_max, int np_max, size_t table_slots);
int unet_instance_overlap(const void *gt_i32, const void *pred_i32, int B, int H, int W, int ng_max, int np_max, size_t table_slots,
                          void *area_gt_u32, void *area_pred_u32, void *match_i32, void *inter_u32, void *status_u64, void *scratch,
                          void *stream);
/* The contingency table of two instance maps restricted to ground-truth foreground: the integers behind the Rand and
 * information scores of the ISBI 2012 challenge (Ronneberger et al. 2015, Table 1; functions.rand_scores).  gt_i32, pred_i32,
 * ng_max, np_max, table_slots and status_u64 as in unet_instance_overlap, with two differences: only pixels with gt >= 1 are
 * counted, and for those pred = 0 ("predicted background") is a column like any other.  A pixel with gt = 0 adds nothing,
 * whatever its pred id, unless an id is out of range: status[b][0] counts such pixels of any gt value.
 *   pair_keys_u64 [table_slots]   : the distinct (b, g, p), g >= 1, p >= 0, packed b << 48 | g << 24 | p, in unspecified order
 *   pair_counts_u32 [table_slots] : the pixels of each
 *   n_pairs_u64 [1]               : how many entries of the two lists are written; the rest is left untouched
 * If status[b][1] != 0 for some b the list misses pixels and the caller repeats the call with a larger table.  Exact integer
 * atomics: after sorting, the list is the same in every run.
 * scratch: unet_partition_pairs_scratch_bytes(B, table_slots), initialised by the call.                                    */
size_t unet_partition_pairs_scratch_bytes(int B, size_t table_slots);
int unet_partition_pairs(const void *gt_i32, const void *pred_i32, int B, int H, int W, int ng_max, int np_max, size_t table_slots,
                         void *pair_keys_u64, void *pair_counts_u32, void *n_pairs_u64, void *status_u64, void *scratch,
                         void *stream);
/* Who touches whom in an instance map, and along how much border (instances.hip; functions.cell_neighbours): for every unordered
 * pair of ids 1 <= i < j of image b, the unit pixel sides at which a pixel of i is 4-adjacent to a pixel of j.  labels,
 * label_dtype, n_max and the limits as unet_cell_sums; outputs, table_slots and the protocol as unet_partition_pairs:
 *   pair_keys_u64 [table_slots]   : the distinct (b, i, j) packed b << 48 | i << 24 | j, in unspecified order
 *   pair_counts_u32 [table_slots] : the sides of each; summed over the pairs that hold i they give unet_cell_sums's contact of i
 *   n_pairs_u64 [1]               : how many entries of the two lists are written; the rest is left untouched
 *   status_u64 [B][2]             : {pixels whose id is outside [0, n_max] (nobody's neighbour);  sides dropped because the table
 *                                    was full: if non-zero the caller repeats the call with a larger table}
 * scratch: unet_cell_contacts_scratch_bytes(B, table_slots), initialised by the call.                                      */
size_t unet_cell_contacts_scratch_bytes(int B, size_t table_slots);
int unet_cell_contacts(const void *labels, int label_dtype, int B, int H, int W, int n_max, size_t table_slots, void *pair_keys_u64,
                       void *pair_counts_u32, void *n_pairs_u64, void *status_u64, void *scratch, void *stream);
/* Linking the cells of consecutive frames by overlap, the greedy tracker of the Cell Tracking Challenge submissions
 * (track.hip; functions.link_frames, functions.track_cells; the definition in full: DESIGN.md section 4s).  from_i32, to_i32
 * id maps int32 [T,H,W], 0 = background, ids anywhere in [0, n_max] (not necessarily consecutive or connected), n_max < 2^24;
 * from_i32 may equal to_i32 (the plain case).  Pair t, 1 <= t < T, sets frame t - 1 of `from` against frame t of `to`.
 *   area_u32 [T][n_max+1]         : pixels per id of `to` (index 0 = background)
 *   pred_i32 [T][n_max+1]         : for t >= 1, c >= 1 the id p >= 1 of from[t-1] with the largest |p n c| > 0, the smallest
 *                                   such p on equal overlaps, 0 when there is none; row 0 and column 0 are 0
 *   pred_overlap_u32 [T][n_max+1] : that |p n c|, else 0
 *   status_u64 [T][2]             : {pixels of pair t with to[t] or (t >= 1) from[t-1] outside [0, n_max] (negative included):
 *                                    used as no index and counted nowhere else, area included;  pixels of pair t dropped because
 *                                    the pair table was full: if non-zero, row t of pred and pred_overlap is invalid and the
 *                                    caller repeats the call with a larger table}
 * table_slots: a power of two, the slots of the open-addressing table of distinct (t, p, c) with p, c >= 1, shared by all frames;
 * a table with more slots than T*H*W cannot fill up.  Five memsets and three launches on the stream, no read-back; exact integer
 * atomics and a 64-bit max of overlap << 24 | (2^24 - 1 - p) per (t, c): results are the same in every run.  T = 1 gives the areas
 * only.  Limits: H * W < 2^31, T <= 65535 (the frame index is the key's top 16 bits).  A NULL pointer, T, H or W < 1, a size over
 * the limit, n_max outside [0, 2^24) and a table_slots that is no power of two return an error and write nothing.
 * scratch: unet_link_frames_scratch_bytes(T, n_max, table_slots) (12 bytes per slot, 8 per (t, id)), initialised by the call. */
size_t unet_link_frames_scratch_bytes(int T, int n_max, size_t table_slots);
int unet_link_frames(const void *from_i32, const void *to_i32, int T, int H, int W, int n_max, size_t table_slots, void *area_u32,
                     void *pred_i32, void *pred_overlap_u32, void *status_u64, void *scratch, void *stream);
/* The graph stage of the Cell Tracking Challenge's DET and TRA measures (AOGM: Matula et al. 2015; aogm.hip; ctc.aogm_counts;
 * the definition in full: DESIGN.md section 4s-ter).  Two time-lapses of id maps labelled by track, the reference ("gt") and the
 * result ("res"), reach this entry as the outputs of one unet_instance_overlap call with B = T on (gt, res): area_gt_u32
 * [T][ng_max+1], area_res_u32 [T][nr_max+1], match_i32 [T][ng_max+1].  No pixel is read here: O(T * (ng_max + nr_max)) work.
 * rows_gt_i32 [ng_max+1][3], rows_res_i32 [nr_max+1][3] (each may be NULL: no table, every label accepted, no parent links):
 * the row (B, E, P) of label L of the challenge's track table, frames counted from 0, P = 0 for "no parent"; B = -1: no row.
 * One side's graph: a vertex is (t, L), L >= 1, with area[t][L] != 0.  Its in-edge comes from L's latest presence before t (kind
 * "track"; it spans the frames in which L is absent), else, at L's first presence with P > 0, from the last presence of P (kind
 * "parent"), else there is none.  A vertex is bad if its label has no row although a table was given, if t is outside [B, E],
 * or if at a first presence with P > 0 the parent is never present (P > n_max included) or its last presence is not before t;
 * a bad parent link gives no in-edge.  Reference vertex g of frame t is matched by m = match[t][g] if m is in [1, nr_max].
 *   claims_u32 [T][nr_max+1]      : the reference vertices of frame t matched by result label s; s is TP iff that is 1
 *   claimant_i32 [T][nr_max+1]    : the largest such reference label (an integer max, so defined for claims > 1 too), 0 if none
 *   inedge_gt_i32 [T][ng_max+1][2], inedge_res_i32 [T][nr_max+1][2] : (frame, label) of the in-edge's source, (-1, 0) if none
 *   flags_gt_u8 [T][ng_max+1], flags_res_u8 [T][nr_max+1] : one byte per (t, L), 0 where there is no vertex.  Both sides:
 *       1 = present, 2 = has an in-edge, 4 = that edge is of kind parent, 8 = bad.  Reference: 16 = matched, 32 = EA (has an
 *       in-edge u -> v that is not reproduced: match(v) = s and match(u) = r both TP and the in-edge of s comes from r), 64 = EC
 *       (reproduced, but the two kinds differ).  Result: 16 = TP, 32 = FP (claims = 0), 64 = ED (has an in-edge r -> s, s and r
 *       both TP, and the in-edge of s's partner does not come from r's partner)
 *   counts_u64 [T][12]            : per frame {n_ref, n_res, e_ref, e_res, TP, FN, FP, NS, EA, ED, EC, bad}: vertices and
 *       in-edges (booked to the frame of their head) of either side, TP result vertices, reference vertices without a match,
 *       result vertices with claims = 0, the sum of claims - 1 over result vertices with claims > 1, the three edge flags, and
 *       the bad vertices of both sides
 * Three launches on the stream, no memset, no read-back; integer atomics only: every output is the same in every run.
 * Limits: 1 <= T <= 65535, ng_max and nr_max in [0, 2^24).  A NULL pointer (the two row arrays apart) or a broken limit returns
 * an error and writes nothing.  Whatever the input words hold, nothing outside the buffers is touched.
 * scratch: unet_aogm_counts_scratch_bytes(T, ng_max, nr_max) (4 bytes per (t, L) and 4 per L of either side), initialised by the
 * call; 0 on a size outside the limits.                                                                                     */
size_t unet_aogm_counts_scratch_bytes(int T, int ng_max, int nr_max);
int unet_aogm_counts(const void *area_gt_u32, const void *area_res_u32, const void *match_i32, const void *rows_gt_i32,
                     const void *rows_res_i32, int T, int ng_max, int nr_max, void *claims_u32, void *claimant_i32, void *inedge_gt_i32,
                     void *inedge_res_i32, void *flags_gt_u8, void *flags_res_u8, void *counts_u64, void *scratch, void *stream);
/* Nearest-cell growth of an instance map (border thinning; skimage.segmentation.expand_labels with an exact metric and a
 * stated tie rule; functions.grow_cells).  labels_i32, out_i32 int32 [B,H,W], 0 = background, ids in [1, 2^24), not
 * necessarily consecutive or connected; H != W allowed, down to 1 x 1.  A pixel with id != 0 keeps it.  A background pixel takes
 * the id of the labelled pixel at the smallest exact squared Euclidean distance d^2 (an integer), the smallest id among those at
 * that d^2.  max_dist2 >= 0: only labelled pixels with d^2 <= max_dist2 count and a pixel with none in reach stays 0 (0 is the
 * identity); max_dist2 < 0: unlimited, and an image without labels stays 0.  A value outside [0, 2^24) is copied to the output
 * and is no cell to grow from (it indexes nothing).  Exact; H * W * min(W, 2 floor(sqrt(max_dist2)) + 257) key evaluations,
 * whatever the number of cells.  Limits as unet_label_components (H * W < 2^31, H <= 65535, B <= 65535) and W <= 65535.
 * scratch: unet_grow_labels_scratch_bytes(B, H, W) (8 bytes per pixel), initialised by the call.                           */
size_t unet_grow_labels_scratch_bytes(int B, int H, int W);
int unet_grow_labels(const void *labels_i32, int B, int H, int W, long long max_dist2, void *out_i32, void *scratch, void *stream);
/* The topology-preserving warp behind the warping error of the ISBI 2012 challenge (Jain et al. 2010; Ronneberger et al. 2015,
 * Table 1; functions.warp_labels, functions.warping_error; the definition in full: DESIGN.md section 4m).  L starts as the ground
 * truth gt, T is the prediction pred; foreground = value != 0, 4-connected, the background 8-connected.  A pixel is a candidate
 * when it is not in the first or last row or column, may flip, and has L != T; it is simple when, among its 8 neighbours in L,
 * the foreground forms exactly one 4-connected component that holds a 4-neighbour of the pixel and the background exactly one
 * 8-connected component.  Pass s = 0..3 flips, at once, every simple candidate with (y & 1) * 2 + (x & 1) == s; a sweep is the
 * passes 0, 1, 2, 3; sweeps repeat until one flips nothing.  connectivity 8 (foreground 8-, background 4-connected) is the same
 * warp of the complements of gt and pred.  Three calls, all on one stream, none of which synchronises:
 *   unet_warp_init    gt, pred, mask [B,H,W] of dtype 0 = int64, 1 = float32, 2 = int32, 3 = uint8 (mask may be NULL: every
 *                     pixel).  max_dist2 >= 0: only pixels whose exact squared distance to the nearest pixel of the other class
 *                     of gt is <= max_dist2 may flip (none in a one-class image; two calls of unet_grow_labels); < 0: no
 *                     such limit.  state_u8 [B,H,W] receives one byte per pixel: bit 0 = L, bit 1 = T (both complemented for
 *                     connectivity 8), bit 2 = may flip (mask AND reach AND not on the image border).  mismatch_before_u32 [B] =
 *                     |gt != pred|.
 *   unet_warp_sweeps  enqueues n_launches launches of passes_per_launch = 4, 8 or 16 passes each (1, 2 or 4 whole sweeps, by
 *                     temporal blocking: the result is that of the passes one by one) on state_u8, in place as the caller sees
 *                     it.  flips_out_u32 [slots][4][B]: launch l of the call first clears, then fills slot first_slot + l:
 *                     [q][b] = the pixels of image b flipped by the q-th sweep of that launch (q < passes_per_launch / 4, the
 *                     rest 0); other slots are untouched.  A launch that flips nothing leaves the state as it is, and so does
 *                     every launch after it: the caller reads the slots back and stops at the first that is all 0.
 *   unet_warp_finish  warped_i32 [B,H,W] = L in {0,1} (complemented back for connectivity 8), mismatch_map_f32 [B,H,W] = 1.0
 *                     where L != T else 0.0 (a mask unet_label_components takes), mismatch_u32 [B] = |L != T|.
 * Exact integers throughout.  Limits as unet_grow_labels (H * W < 2^31, H, W, B <= 65535), H != W allowed, down to 1 x 1.
 * scratch: unet_warp_scratch_bytes(B, H, W), the same buffer for unet_warp_init and every unet_warp_sweeps of one warp (it holds
 * the second state plane; 21 bytes per pixel).                                                                              */
size_t unet_warp_scratch_bytes(int B, int H, int W);
int unet_warp_init(const void *gt, int gt_dtype, const void *pred, int pred_dtype, const void *mask, int mask_dtype, int B, int H, int W,
                   long long max_dist2, int connectivity, void *state_u8, void *mismatch_before_u32, void *scratch, void *stream);
int unet_warp_sweeps(void *state_u8, int B, int H, int W, int passes_per_launch, int n_launches, void *flips_out_u32, int first_slot,
                     void *scratch, void *stream);
int unet_warp_finish(const void *state_u8, int B, int H, int W, int connectivity, void *warped_i32, void *mismatch_map_f32,
                     void *mismatch_u32, void *stream);
/* Seeded geodesic growth inside a mask: split touching cells by growing confident cores back inside the mask until two growths
 * meet (functions.split_cells, tester.split_instances; the definition in full: DESIGN.md section 4n).  The region is mask != 0.
 * g(p) is the least number of 4-neighbour steps from a seed pixel to p along region pixels, 0 on a seed pixel.  A region pixel
 * with g(p) <= max_steps takes the id of the seed pixel at distance g(p), the smallest id among those at that distance (the tie
 * rule of unet_grow_labels with the geodesic metric); every other pixel, a seed pixel outside the region included, gets 0.
 * max_steps < 0: unlimited; 0: the seeds restricted to the region.  Three calls, all on one stream, none of which synchronises:
 *   unet_geodesic_init    seeds_i32 [B,H,W], 0 = no seed, ids in [1, 2^24); mask [B,H,W] of dtype 0 = int64, 1 = float32,
 *                         2 = int32, 3 = uint8.  Writes one 64-bit key per pixel into the scratch (distance << 24 | id, or a code
 *                         for "outside the region" or "region, not reached yet": the mask is not read again).
 *                         seeds_outside_u32 [B] = the seed pixels outside the region; status_u64 [B] = the pixels whose seed id is
 *                         outside [0, 2^24): such a value indexes nothing, is no seed and is in neither count above.
 *   unet_geodesic_sweeps  enqueues n_launches launches.  In each, a workgroup relaxes its 64 x 64 tile, staged with a halo of one
 *                         pixel, to local convergence and hands off to its neighbours at the kernel boundary (two key planes,
 *                         ping-pong), so a growth needs about as many launches as its longest shortest path crosses tile borders.
 *                         changed_out_u32 [slots][B]: launch l of the call first clears, then fills slot first_slot + l:
 *                         [b] = the pixels of image b whose key that launch lowered; other slots are untouched.  A launch that
 *                         changes nothing leaves the state as it is, and so does every launch after it: the caller reads the slots
 *                         back and stops at the first that is all 0.  max_steps >= 0 prunes keys beyond it and changes no key
 *                         with a distance <= max_steps; pass the same value to unet_geodesic_finish.
 *   unet_geodesic_finish  out_i32 [B,H,W] = the ids; dist_i32 [B,H,W] (may be NULL) = g(p), -1 where out is 0;
 *                         unreached_u32 [B] = the region pixels with out = 0; max_dist_u32 [B] = the largest g written, 0 when
 *                         there is none.
 * Exact integers throughout: any order of relaxation reaches the same fixed point.  Limits as unet_grow_labels (H * W < 2^31,
 * H, W, B <= 65535), H != W allowed, down to 1 x 1.
 * scratch: unet_geodesic_scratch_bytes(B, H, W), the same buffer for the three calls of one growth (the two key planes; 16 bytes
 * per pixel), initialised by unet_geodesic_init.                                                                            */
size_t unet_geodesic_scratch_bytes(int B, int H, int W);
int unet_geodesic_init(const void *seeds_i32, const void *mask, int mask_dtype, int B, int H, int W, void *seeds_outside_u32,
                       void *status_u64, void *scratch, void *stream);
int unet_geodesic_sweeps(int B, int H, int W, long long max_steps, int n_launches, void *changed_out_u32, int first_slot, void *scratch,
                         void *stream);
/* The four sweep entries with a connectivity, 4 or 8 (after unet_label_components_conn): unet_geodesic_sweeps_conn,
 * unet_flood_sweeps_conn, unet_flood_assign_conn and unet_reconstruct_sweeps_conn are the entries without _conn with
 * `int connectivity` directly before n_launches, and the entries without _conn are these with 4.  With 8 a step goes to any of
 * the eight neighbours that lies in the region, whatever the two pixels beside a diagonal step are (a one-pixel-thick diagonal
 * wall does not separate): g(p) counts 8-neighbour steps, the flood's minimum runs over eight neighbours and a parent is any of
 * the eight whose key extends to exactly key(q), and R(p) >= min(under(p), R(n)) holds for every region 8-neighbour n.  init,
 * finish and the scratch sizes do not depend on it; both stages of one flood take the same value.  Anything but 4 or 8 returns -2
 * with a unet_last_error() that names it, and enqueues nothing.                                                              */
int unet_geodesic_sweeps_conn(int B, int H, int W, long long max_steps, int connectivity, int n_launches, void *changed_out_u32,
                              int first_slot, void *scratch, void *stream);
int unet_flood_sweeps_conn(int B, int H, int W, long long max_level, int connectivity, int n_launches, void *changed_out_u32, int first_slot,
                           void *scratch, void *stream);
int unet_flood_assign_conn(int B, int H, int W, int connectivity, int n_launches, void *changed_out_u32, int first_slot, void *scratch,
                           void *stream);
int unet_reconstruct_sweeps_conn(int B, int H, int W, int connectivity, int n_launches, void *changed_out_u32, int first_slot, void *scratch,
                                 void *stream);
int unet_geodesic_finish(int B, int H, int W, long long max_steps, void *out_i32, void *dist_i32, void *unreached_u32, void *max_dist_u32,
                         void *scratch, void *stream);
/* Seeded watershed: flooding of an intensity landscape from markers inside a region (functions.watershed,
 * tester.split_by_watershed; the definition in full: DESIGN.md section 4r).  The region is mask != 0, or every pixel when mask is
 * NULL.  Every pixel has a level v in [0, 65536); a seed pixel inside the region is a source with key (L, d) = (0, 0); one
 * 4-neighbour step onto a region pixel q turns a key (L, d) into (L, d + 1) if v(q) <= L and into (v(q), 1) otherwise.  Stage 1:
 * key(q) = the lexicographic minimum over all region paths from a source (L the pass height at which the flood reaches q, d the
 * steps inside the plateau of that height).  Stage 2: neighbour p is a parent of q when its key extends to exactly key(q); a source
 * keeps its id, every other reached pixel takes the least id among its parents.  Unreached pixels, pixels with L > max_level and
 * pixels outside the region get 0.  On a constant image this is unet_geodesic_*'s growth bit for bit.  Five calls, all on one
 * stream, none of which synchronises:
 *   unet_flood_init    seeds_i32 [B,H,W], 0 = no seed, ids in [1, 2^24); image [B,H,W] of image_dtype 0 = int64, 1 = float32,
 *                      2 = int32, 3 = uint8; mask [B,H,W] (may be NULL) of mask_dtype with the same codes.  Integer images are
 *                      read as they are; a float32 image needs levels in [1, 65536] and gives
 *                      v = min(levels - 1, max(0, floorf(x * (float)levels))), the product in fp32.  Writes the level plane
 *                      (uint16), the key plane (L << 32 | d, or a code for "outside the region" or "not reached yet") and the id
 *                      plane into the scratch; neither input is read again.  seeds_outside_u32 [B] = the seed pixels outside the
 *                      region; status_u64 [2][B]: [0][b] = the pixels whose seed id is outside [0, 2^24) (no seed, in no other
 *                      count), [1][b] = the pixels whose image value is outside [0, 65536) or not finite (read as level 0).
 *   unet_flood_sweeps  stage 1, the protocol of unet_geodesic_sweeps: enqueues n_launches launches, in each a workgroup relaxes its
 *                      64 x 64 tile to local convergence and hands off at the kernel boundary (two key planes, ping-pong);
 *                      changed_out_u32 [slots][B]: launch l first clears, then fills slot first_slot + l with the pixels whose
 *                      key it lowered; other slots are untouched.  A launch that changes nothing leaves the state as it is, and
 *                      so does every launch after it.  max_level < 0: unlimited; else keys with L > max_level are never stored,
 *                      which changes no key with L <= max_level.
 *   unet_flood_assign  stage 2, the same protocol over the two id planes (the slots count the ids lowered).  It takes on trust
 *                      that the keys are final: call it only after the caller has SEEN a launch of unet_flood_sweeps that changed
 *                      nothing, and call unet_flood_sweeps no more afterwards.  On keys that are not final the ids it leaves are
 *                      those of no definition.
 *   unet_flood_finish  call it after a launch of unet_flood_assign that changed nothing.  out_i32 [B,H,W] = the ids;
 *                      pass_level_i32 and dist_i32 [B,H,W] (each may be NULL) = L and d, -1 where out is 0; unreached_u32 [B] =
 *                      the region pixels with out = 0; max_level_u32 [B] = the largest L written, 0 when there is none.
 * Exact integers throughout: any order of relaxation reaches the same fixed point in either stage.  Limits as unet_grow_labels
 * (H * W < 2^31, H, W, B <= 65535), H != W allowed, down to 1 x 1.
 * scratch: unet_flood_scratch_bytes(B, H, W), the same buffer for all calls of one flooding: two planes of 64-bit keys, two
 * planes of 32-bit ids and the plane of 16-bit levels, 26 bytes per pixel (each plane rounded up to 256 bytes), initialised by
 * unet_flood_init.                                                                                                          */
size_t unet_flood_scratch_bytes(int B, int H, int W);
int unet_flood_init(const void *seeds_i32, const void *image, int image_dtype, int levels, const void *mask, int mask_dtype, int B, int H,
                    int W, void *seeds_outside_u32, void *status_u64, void *scratch, void *stream);
int unet_flood_sweeps(int B, int H, int W, long long max_level, int n_launches, void *changed_out_u32, int first_slot, void *scratch,
                      void *stream);
int unet_flood_assign(int B, int H, int W, int n_launches, void *changed_out_u32, int first_slot, void *scratch, void *stream);
int unet_flood_finish(int B, int H, int W, void *out_i32, void *pass_level_i32, void *dist_i32, void *unreached_u32, void *max_level_u32,
                      void *scratch, void *stream);
/* Seeds from the shape of a mask alone: the distance map of the region, its h-maxima, the domes that are left
 * (functions.distance_map, functions.reconstruct, functions.shape_seeds, tester.split_by_shape; the definitions in full: DESIGN.md
 * section 4o).  The region is mask != 0; mask [B,H,W] of dtype 0 = int64, 1 = float32, 2 = int32, 3 = uint8.  None of these
 * calls synchronises; exact integers throughout.  Limits: H, W <= 32767, H * W < 2^31, B <= 65535; H != W allowed, down to 1 x 1.
 *
 * unet_distance_map: d2_i32 [B,H,W] = the exact squared Euclidean distance from a region pixel to the nearest pixel outside the
 * region, 0 outside the region.  edge 0 ("ignore", scipy.ndimage.distance_transform_edt's convention): there is nothing past the
 * image, and an image without a pixel outside the region gets H^2 + W^2 everywhere, which is above every real value.  edge 1
 * ("background"): every pixel past the image is outside the region, so the pixel in row y and column x is at most
 * min(x + 1, W - x, y + 1, H - y) away from one.  A column pass and a row pass whose scan outwards ends once dx^2 reaches the
 * running minimum.  scratch: unet_distance_map_scratch_bytes(B, H, W) (4 bytes per pixel), initialised by the call.
 *
 * Grey reconstruction by dilation, 4-connected: marker and under [B,H,W] of dtype 0 = int64 or 2 = int32 with values in
 * [0, 2^30]; the region is mask != 0, every pixel when mask is NULL.  R is the least function on the region with
 * R >= min(marker, under), R <= under and R(p) >= min(under(p), R(n)) for every region 4-neighbour n; equivalently R(p) is the
 * maximum over region pixels q of min(marker(q), the minimum of under along the best 4-path from q to p inside the region).
 * Three calls, all on one stream:
 *   unet_reconstruct_init    writes R = min(marker, under) and under into the scratch, -1 outside the region (the mask is not
 *                            read again).  status_u64 [B] = the pixels, inside the region or not, where marker or under is outside
 *                            [0, 2^30]: such a value counts as 0.
 *   unet_reconstruct_sweeps  enqueues n_launches launches.  In each, a workgroup relaxes its 64 x 64 tile, staged with a halo of
 *                            one pixel, to local convergence of R <- min(under, max(R, the four neighbours)) and hands off to its
 *                            neighbours at the kernel boundary (two planes, ping-pong).  changed_out_u32 [slots][B]: launch l of
 *                            the call first clears, then fills slot first_slot + l: [b] = the pixels of image b that launch
 *                            raised; other slots are untouched.  A launch that raises nothing leaves the state as it is, and so
 *                            does every launch after it: the caller reads the slots back and stops at the first that is all 0.
 *   unet_reconstruct_finish  out_i32 [B,H,W] = R, 0 outside the region; raised_u32 [B] = the pixels with R > min(marker, under).
 * Values only rise and every value held is a lower bound of R: any order of relaxation reaches the same fixed point.
 * scratch: unet_reconstruct_scratch_bytes(B, H, W), the same buffer for the three calls of one reconstruction (two planes of R,
 * under, and min(marker, under); 16 bytes per pixel), initialised by unet_reconstruct_init.
 *
 * The element-wise steps of functions.shape_seeds, on int32 [B,H,W]:
 *   unet_shape_heights  q_i32 = floor(sqrt(256 d2)), the floor of the distance in 1/16 pixel, exactly; lifted_i32 (may be NULL)
 *                       = q + hq, 0 <= hq <= 2^28
 *   unet_shape_lower    out_i32 = max(in - c, 0), c >= 0
 *   unet_shape_maxima   out_f32 = 1.0 where r2 < r1 and r1 >= floor_q, else 0.0 (a mask unet_label_components takes): with
 *                       r2 = the reconstruction of max(r1 - 1, 0) under r1, the regional maxima of r1 that reach floor_q      */
size_t unet_distance_map_scratch_bytes(int B, int H, int W);
int unet_distance_map(const void *mask, int mask_dtype, int B, int H, int W, int edge, void *d2_i32, void *scratch, void *stream);
size_t unet_reconstruct_scratch_bytes(int B, int H, int W);
int unet_reconstruct_init(const void *marker, int marker_dtype, const void *under, int under_dtype, const void *mask, int mask_dtype, int B,
                          int H, int W, void *status_u64, void *scratch, void *stream);
int unet_reconstruct_sweeps(int B, int H, int W, int n_launches, void *changed_out_u32, int first_slot, void *scratch, void *stream);
int unet_reconstruct_finish(int B, int H, int W, void *out_i32, void *raised_u32, void *scratch, void *stream);
int unet_shape_heights(const void *d2_i32, int B, int H, int W, int hq, void *q_i32, void *lifted_i32, void *stream);
int unet_shape_lower(const void *in_i32, int B, int H, int W, int c, void *out_i32, void *stream);
int unet_shape_maxima(const void *r1_i32, const void *r2_i32, int B, int H, int W, int floor_q, void *out_f32, void *stream);
/* Carved training targets from an instance image, replaces preprocess_gt (data.py:195-221: per cell, cv.dilate with a 5 x 5
 * rectangle, iterations=2, and 255 added on the ring the cell gained) and the cv.threshold(gt, 0, 255, THRESH_BINARY) after it
 * (data.py:64, :163).  ids [B,H,W], dtype 0 = int64, 1 = float32 holding integral values, 2 = int32 (what
 * unet_label_components writes); 0 = background, objects any ids in [1, 2^24), not necessarily consecutive or connected; H != W
 * allowed, down to 1 x 1.  reach = iterations * (kernel - 1) / 2 (4 for the reference), 0 <= reach <= 8: the iterated
 * rectangles are one (2 reach + 1)^2 rectangle clipped to the image.  With n(p) = the number of distinct ids other than 0 and
 * id(p) in that window around p:
 *   edges_f32 [B,H,W] = 255 n           (mask_global)
 *   gt_f32    [B,H,W] = max(0, id - 255 n)
 *   bin_u8    [B,H,W] = 255 where gt > 0, else 0
 * each may be NULL, not all three.  Every value is an integer below 2^24, exact in fp32.  status_u64 [B] = pixels whose id is
 * outside [0, 2^24) (negative and NaN included): such a pixel is background everywhere and indexes nothing.  Exact; the cost
 * depends on reach and on the image size, never on the number of cells.  No scratch.                                        */
int unet_carve_borders(const void *ids, int dtype, int B, int H, int W, int reach, void *gt_f32, void *edges_f32, void *bin_u8,
                       void *status_u64, void *stream);
/* The integers behind the weighted crop distribution, replaces the np.mean(gt_bin[ii:ii+crop, jj:jj+crop]) of every window of
 * ImageDataset.__init__ (data.py:67-82).  mask [B,H,W], dtype 0 = int64, 1 = float32, 2 = int32, 3 = uint8; foreground =
 * value != 0.  counts_u32 [B][ny][nx], ny = ceil((H - crop) / skip), nx = ceil((W - crop) / skip) (= len(range(0, H - crop,
 * skip)), ...): counts[b][i][j] = foreground pixels of rows [skip i, skip i + crop) x columns [skip j, skip j + crop).  Exact,
 * from per-row prefix sums: no pixel is read once per window.  H <= crop, W <= crop, crop < 1 or skip < 1 leave the reference
 * no window to draw from: UNET_E_BADARG (and 0 scratch bytes).  H * W < 2^31.
 * scratch: unet_crop_counts_scratch_bytes(B, H, W, crop, skip), initialised by the call.                                   */
size_t unet_crop_counts_scratch_bytes(int B, int H, int W, int crop, int skip);
int unet_crop_counts(const void *mask, int dtype, int B, int H, int W, int crop, int skip, void *counts_u32, void *scratch,
                     void *stream);
/* N1, replaces elastic_transform's two steps (data.py:225-245): scipy.ndimage.gaussian_filter(field,
 * sigma, mode="constant") * scale as two 1-D passes with the caller's normalised taps [2*radius+1], and
 * map_coordinates(img, (row+dy, col+dx), order=1) (bilinear, 0 outside [0,n-1]).                       */
int unet_gaussian_filter(const void *field, int B, int H, int W, const void *weights, int radius, float scale,
                         void *tmp, void *out, void *stream);
int unet_warp_bilinear(const void *img, const void *dy, const void *dx, int B, int H, int W, void *out, void *stream);
/* N1, replaces the reflect pad + random rotation + centre crop of ImageDataset.__getitem__ (data.py:108-125):
 *   np.pad(image, pad, 'reflect') -> scipy.ndimage.rotate(deg) (cubic spline, reshape=True, 'constant') -> [t:b, l:r] (S x S),
 * fused so that only the pixels the crop samples are formed.  img fp32 [B,n,n] (n = the random crop, e.g. 388), pad = the
 * np.pad width (the reference passes input_size = S), angles: HOST array of B degrees, out fp32 [B,S,S].
 * levels: 0 keeps the float result; 255 / 65535 reproduce scipy's conversion for the uint8 / uint16 images the reference
 * loads: (type)min(t > 0 ? t + 0.5 : 0, levels) (scipy 1.15).  scratch >= unet_rotate_scratch_bytes(B, S).             */
size_t unet_rotate_scratch_bytes(int B, int S);
int unet_reflect_rotate_crop(const void *img, int B, int n, int pad, int S, const float *angles_deg_host, int levels,
                             void *out, void *scratch, void *stream);
/* The paper's elastic deformation (Ronneberger et al. §3.1): per sample a coarse displacement grid g [2,G,G]
 * fp64 in pixels (plane 0 displaces rows, plane 1 columns; 2 <= G <= UNET_ELASTIC_MAX_GRID), corner-aligned on the H x W
 * sample (row y sits at grid position y (G-1)/(H-1)), interpolated to every pixel with Keys' cubic convolution of parameter a
 * (-0.5: Keys' third-order kernel; -0.75: torch's bicubic), node indices clamped to [0, G-1]; the planes are then sampled at
 * (y + d_row, x + d_col) as unet_warp_bilinear samples (bilinear inside [0,H-1] x [0,W-1], 0 outside).  Displacement,
 * coordinate and bilinear combination are fp64 on the device, narrowed to fp32 at the store; no field is ever stored.
 * grid_f64: DEVICE fp64 [B,2,G,G].  H, W >= 2.
 *   unet_elastic_grid        : planes fp32 [P,B,H,W] -> out fp32 [P,B,H,W], every plane of sample b warped with grid b; one
 *                              launch, no rounding.
 *   unet_elastic_grid_sample : the training sample.  img, mask fp32 [B,S,S]; out_img fp32 [B,S,S] = the warped image,
 *                              rounded for levels = 255 / 65535 as the reference's integer images round (floor(v + 0.5)
 *                              clamped to [0, levels]; levels = 0 keeps the float value); minmax fp32 [B][2] = each
 *                              sample's min and max of out_img; out_gt_i64 [B,crop,crop] = (the mask warped with the same
 *                              grid and rounded the same way) > 127, formed for the window [pad, pad+crop)^2 only
 *                              (pad >= 0, crop >= 1, pad + crop <= S).
 *   unet_normalise01         : x fp32 [B][n] in place: (x - lo) / (hi - lo) with lo, hi = minmax[b] (fp32, true division;
 *                              hi == lo gives 0/0 = NaN, as the expression does).                                          */
#define UNET_ELASTIC_MAX_GRID 16
int unet_elastic_grid(const void *planes, int P, int B, int H, int W, const void *grid_f64, int G, double a, void *out, void *stream);
int unet_elastic_grid_sample(const void *img, const void *mask, int B, int S, const void *grid_f64, int G, double a, int levels,
                             int pad, int crop, void *out_img, void *out_gt_i64, void *minmax, void *stream);
int unet_normalise01(void *x, int B, size_t n, const void *minmax, void *stream);
/* Grey-value variation of training samples (Ronneberger et al. §3.1 names it beside shift, rotation and deformation; the
 * reference has none).  x fp32 [B][n] -> out fp32 [B][n], out == x (in place) or disjoint from x.  Sample b has five
 * HOST parameters params_host[5 b ..]: gamma > 0, contrast >= 0, brightness, sigma >= 0, invert (0 or 1), all finite.  Per
 * pixel i of sample b, the stages in this order; everything after the normalisation is fp64, narrowed to fp32 once at the store:
 *   normalise  only with minmax (DEVICE fp32 [B][2], as unet_elastic_grid_sample leaves it): x <- (x - lo) / (hi - lo) in
 *              fp32 with true division, bit-equal to calling unet_normalise01 first
 *   mean       m = (sum_i x[i]) / n, an fp64 sum in a fixed order (per-workgroup partials combined in index order, no
 *              floating-point atomics); formed only for a sample whose affine stage runs
 *   affine     u = (x - m) * contrast + m + brightness, then u = min(max(u, 0), 1): contrast about the sample's own mean
 *   gamma      u = u^gamma, or 1 - (1 - u)^gamma with invert; meant for u in [0,1] (pow of a negative base is NaN)
 *   noise      u += sigma * z, z standard normal by Box-Muller from Philox4x32-10:
 *                counter = (i >> 2, first_sample + b, step lo, step hi),  key = (seed lo, seed hi ^ 0x47524559)
 *                words 0, 1 -> pixels 4g (r cos t) and 4g+1 (r sin t), words 2, 3 -> 4g+2 and 4g+3, with
 *                u1 = (w + 0.5) 2^-32 of the first word, u2 likewise of the second, r = sqrt(-2 log u1), t = 2 pi u2
 *   clip       y = min(max(u, 0), 1) unless flags has UNET_GREY_NO_CLIP
 * A stage whose parameters are the identity is skipped for that sample, not computed: contrast == 1 && brightness == 0,
 * gamma == 1, sigma == 0.  Identity parameters on a [0,1] image return it bit for bit, and a sample without noise never runs
 * Philox.  A NaN is no special case: min and max here keep it, 0/0 of a constant sample's normalisation stays NaN, and a NaN
 * mean makes every pixel of that sample's affine stage NaN.
 * At most UNET_GREY_MAX_SAMPLES samples per call; first_sample is the global index of sample 0, so a batch done in chunks
 * equals one call.  Two launches when any sample needs its mean (partial sums, then the stages), one otherwise; no host sync,
 * bit-identical on every run and stream.  The parameters are checked on the host before anything is enqueued.  1 <= n < 2^31,
 * first_sample + B <= 2^32.  scratch >= unet_grey_scratch_bytes(B, n); it may be NULL when no sample's affine stage runs.
 *   unet_grey_normals : out_f64 DEVICE fp64 [n] = z of pixels [first, first + n) of global sample `sample` (tests).            */
#define UNET_GREY_MAX_SAMPLES 64
#define UNET_GREY_NO_CLIP 1
size_t unet_grey_scratch_bytes(int B, size_t n);
int unet_grey_vary(const void *x, void *out, int B, size_t n, long long first_sample, const double *params_host,
                   const void *minmax_or_null, unsigned long long seed, unsigned long long step, int flags, void *scratch,
                   void *stream);
int unet_grey_normals(unsigned long long seed, unsigned long long step, long long sample, size_t first, size_t n, void *out_f64,
                      void *stream);

/* ---- per-op entry points (NHWC fp32), used by the unit tests ---------------------------------
 * Each replaces the ATen op dispatched at the cited line.  w_* are in reference layout.    */
/* nn.Conv2d(3x3, valid)+ReLU, network.py:131-188.  Second source (x2) is the virtual
 * crop_and_concat (network.py:108-127): x1 = skip [B,H1,W1,C1] zero-padded by pad1 per side,
 * x2 = up-conv output [B,H,W,C2]; pass x2=NULL,C2=0,pad1=0 for a plain conv.  H,W = extent of
 * the (virtual) input; y : [B,H-2,W-2,K].  scratch >= unet_conv3x3_scratch_bytes(C1+C2,K).
 * A single source may carry a signed pad too (x2=NULL, H1 + 2 pad1 == H: zero border for pad1 > 0, crop for pad1 < 0), in
 * the forward and the backward.  With bf16 tensors (arithmetic mode 2) every source needs whole 64-channel tiles, and so
 * does dz for dx / dw; a call outside that is refused before anything is enqueued.                                  */
size_t unet_conv3x3_scratch_bytes(int C, int K);
int unet_conv3x3_fwd(const void *x1, int H1, int W1, int C1, int pad1, const void *x2, int C2,
                     int B, int H, int W, const void *w_oihw, const void *bias, int K, int relu,
                     void *y, void *scratch, void *stream);
/* backward of the same: dz is the gradient w.r.t. the PRE-activation of this conv
 * ([B,H-2,W-2,K]).  Outputs (any may be NULL): dx1 [B,H1,W1,C1] (crop of the padded region),
 * dx2 [B,H,W,C2], dw OIHW, db.  mask1/mask2: if non-NULL, dx is multiplied by (mask>0)
 * (ReLU backward of the producer).  add1: if non-NULL it is added to dx1 (skip gradient).
 * scratch >= unet_conv3x3_bwd_scratch_bytes(B,H,W,C1+C2,K).                                  */
size_t unet_conv3x3_bwd_scratch_bytes(int B, int H, int W, int C, int K);
int unet_conv3x3_bwd(const void *x1, int H1, int W1, int C1, int pad1, const void *x2, int C2,
                     int B, int H, int W, const void *w_oihw, int K, const void *dz,
                     void *dx1, const void *mask1, const void *add1, void *dx2, const void *mask2,
                     void *dw, void *db, void *scratch, void *stream);
/* F.max_pool2d(2,2), network.py:133-151 and its backward fused with the ReLU backward of
 * the pooled tensor's producer: dpre = route(dy) * (pre > 0).                              */
int unet_maxpool2_fwd(const void *x, void *y, int B, int H, int W, int C, void *stream);
int unet_maxpool2_bwd(const void *pre, const void *dy, void *dpre, int B, int H, int W, int C,
                      void *stream);
/* Drop-out (Ronneberger et al. 2015, section 3.1; flags and arithmetic as stated at unet_forward_dropout) of x [B,H,W,C] in
 * place and, unless pooled is NULL, F.max_pool2d(2,2) of the dropped tensor into pooled [B,H/2,W/2,C]; its backward:
 * g[0,n) *= 1 / (1 - p) in place.  H, W even, C % 4 == 0, 0 <= p < 1, site 0 or 1.                                    */
int unet_dropout_pool_fwd(void *x_inout, void *pooled_or_null, int B, int H, int W, int C, float p,
                          unsigned long long seed, unsigned long long step, int site, void *stream);
int unet_dropout_bwd(void *g_inout, size_t n, float p, void *stream);
/* nn.ConvTranspose2d(k2,s2), network.py:159-183: x [B,H,W,Ci] -> y [B,2H,2W,Co]; w IOHW.
 * The forward takes H != W; the backward takes square tiles only (H == W, checked).       */
size_t unet_upconv2_scratch_bytes(int B, int H, int W, int Ci, int Co);
int unet_upconv2_fwd(const void *x, int B, int H, int W, int Ci, const void *w_iohw,
                     const void *bias, int Co, void *y, void *scratch, void *stream);
int unet_upconv2_bwd(const void *x, int B, int H, int W, int Ci, const void *w_iohw, int Co,
                     const void *dy, void *dx, const void *mask, void *dw, void *db,
                     void *scratch, void *stream);
/* finalconv 1x1 (network.py:190): x NHWC [B,H,W,C] -> logits NCHW [B,2,H,W]; and backward:
 * dz = (dlogits . W) * (x > 0) (x is the ReLU output of conv12e), dw [2,C,1,1], db [2].     */
int unet_head1x1_fwd(const void *x, int B, int H, int W, int C, const void *w, const void *bias,
                     void *logits, void *stream);
size_t unet_head1x1_bwd_scratch_bytes(int B, int H, int W, int C);
int unet_head1x1_bwd(const void *x, int B, int H, int W, int C, const void *w,
                     const void *dlogits, void *dz, void *dw, void *db, void *scratch,
                     void *stream);
/* finalconv of a K-class net (2 <= K <= 16): logits NCHW [B,K,H,W]; backward dz = (sum_k dl_k w_k) * (x > 0), dw [K,C,1,1] and
 * db [K] from fixed-order per-block partials.  K = 2 runs the head1x1 kernels above (bit-identical to them).  */
int unet_head1xk_fwd(const void *x, int B, int H, int W, int C, int K, const void *w, const void *bias, void *logits, void *stream);
size_t unet_head1xk_bwd_scratch_bytes(int B, int H, int W, int C, int K);
int unet_head1xk_bwd(const void *x, int B, int H, int W, int C, int K, const void *w, const void *dlogits, void *dz, void *dw, void *db,
                     void *scratch, void *stream);
/* conv11c (network.py:23,131): the 1->K stencil layer, direct HBM-bound kernel.
 * x [B,S,S] -> y [B,S-2,S-2,K] (+ReLU); backward gives dw [K,1,3,3], db [K] only.          */
int unet_conv1ch_fwd(const void *x, int B, int S, const void *w, const void *bias, int K,
                     void *y, void *stream);
size_t unet_conv1ch_bwd_scratch_bytes(int B, int S, int K);
int unet_conv1ch_bwd(const void *x, int B, int S, int K, const void *dz, void *dw, void *db,
                     void *scratch, void *stream);
/* its input gradient alone (what unet_backward_input runs on the whole net): dz [B,S-2,S-2,K] -> dx [B,S,S] fp32,
 * dx[b][y][x] = sum_{k,ty,tx} dz[b][y-ty][x-tx][k] w[k][ty][tx] (full correlation with the flipped filter); no scratch. */
int unet_conv1ch_dgrad(const void *dz, int B, int S, int K, const void *w, void *dx, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* UNET_HIP_H */
