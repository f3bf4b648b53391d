/*
 * trainner_hip.h -- C ABI of libtrainner_hip.so: the MI355X (gfx950) kernels behind the
 * ESRGAN/RRDBNet SR training step of victorca25/traiNNer.
 *
 * The reference has NO native boundary (it is 100 % Python on stock ATen kernels), so this ABI
 * is the boundary a maintainer would bind with ctypes.  Every entry point
 * names the reference call site whose arithmetic it replaces; paths are relative to
 * /root/reference/codes.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.  All pointers are DEVICE pointers
 *     owned by the caller; nothing is allocated inside (workspaces are passed in explicitly).
 *   - every call is asynchronous on the hipStream_t passed as `stream` (void*; 0 = null stream).
 *   - return value: 0 = ok, negative = TNR_E*; tnr_last_error() gives a message.
 *   - activations are fp32 NHWC "views": element (n,y,x,c) of a view lives at
 *         ptr[ ((n*H + y)*W + x) * ctot + coff + c ]
 *     so a dense-block buffer (ctot = 192) is addressed in place -- torch.cat
 *     (RRDBNet_arch.py:152-160) never materialises.  ctot and coff are multiples of 4.
 *   - weights cross the boundary in PyTorch's OIHW layout (state_dict compatible) and are
 *     re-laid out on device by tnr_pack_weights into the K-chunked [tap][kout][kin] form.
 */
#ifndef TRAINNER_HIP_H
#define TRAINNER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TNR_OK 0
#define TNR_EINVAL (-1)   /* bad argument / unsupported shape */
#define TNR_ELAUNCH (-2)  /* HIP launch / runtime error */

enum { TNR_ACT_NONE = 0, TNR_ACT_LRELU = 1, TNR_ACT_RELU = 2 };

/* conv geometries on the path */
enum {
    TNR_CONV_3x3 = 0,      /* k3 s1 p1: every G / VGG conv, D odd layers (block.py:214-256)              */
    TNR_CONV_3x3_UP2 = 1,  /* nearest x2 (block.py:326-371,390-404) folded into the k3 s1 p1 gather       */
    TNR_CONV_4x4_S2 = 2,   /* k4 s2 p1: Discriminator_VGG even layers (discriminators.py:24-34)           */
    TNR_DGRAD_4x4_S2 = 3,  /* data-gradient of k4 s2 p1 (aten convolution_backward), parity-decomposed    */
    TNR_CONV_1x1 = 4,      /* k1 s1: the GEMM behind tnr_im2col for the small-spatial layers of the       */
                           /* discriminator tail (discriminators.py:24-36 at 16x16 and below)             */
    TNR_CONV_3x3_C4 = 5,   /* k3 s1 p1 over a <= 4-channel NHWC4 image (VGG conv1_1, D conv0, and the     */
                           /* data-gradient of G's last conv): the 9 taps are folded into K = 36 -> 48    */
                           /* inside the stager instead of padding 3 channels to 16 per tap               */
    TNR_CONV_7x7_C4 = 6    /* k7 s1 p3 over a <= 4-channel NHWC4 image (ResnetGenerator's first layer,    */
                           /* ResNet_arch.py:52-55, and the data-gradient of its last, :86-88): the 49    */
                           /* taps folded into K = 196 -> 208; pad_mode 1 = ReflectionPad2d(3)            */
};

/* weight packings produced by tnr_pack_weights */
enum {
    TNR_PACK_FWD = 0,       /* [kh*kw][KoutP][KinP]            <- W[co][ci][ky][kx]                         */
    TNR_PACK_DGRAD_3x3 = 1, /* [9][KoutP=ci][KinP=co]          <- W[co][ci][2-ky][2-kx]                     */
    TNR_PACK_FWD_S2D = 2,   /* [4][KoutP][4*KinP] (space-to-depth view of k4 s2)                           */
    TNR_PACK_DGRAD_S2 = 3,  /* [4 parities][4][KoutP=ci][KinP=co]                                          */
    TNR_PACK_COL_FWD = 4,   /* [1][KoutP][KinP = kh*kw*Cin]: column (ky*kw+kx)*Cin+ci of tnr_im2col          */
    TNR_PACK_COL_DGRAD3 = 5,/* [1][KoutP=ci][KinP = k*k*Cout]: column t*Cout+co <- W[co][ci][k-1-ty][k-1-tx]  */
                            /* (any square k: the stride-1 data-gradient as im2col(g, pad k-1-p) x this)   */
    TNR_PACK_C4_FWD = 6,    /* [1][KoutP][48]: column 4*t + ci (Cin <= 4)        for TNR_CONV_3x3_C4             */
    TNR_PACK_C4_DGRAD3 = 7, /* [1][KoutP=ci][48]: column 4*t + co (Cout <= 4), taps flipped                     */
                            /* (both also with kh = kw = 7: [..][208] for TNR_CONV_7x7_C4)                     */
    /* A 3x3 layer behind nearest x2 (block.py:326-371) as the virtual 4x4 s2 p1 convolution S it is the data-gradient of:
     * W_S[ci][co][ky][kx] = sum of W[co][ci][ty][tx] over ty in T(ky), tx in T(kx), T = {2}, {1,2}, {0,1}, {0} (tnr_upconv_fold_table;
     * fp32, added inside a row over ascending tx first, then the rows over ascending ty).  Both are made straight from the 3x3 tensor: */
    TNR_PACK_UP2_DGRAD_S2 = 8, /* TNR_PACK_DGRAD_S2's layout of S, [4 parities][4][KoutP=co][KinP=ci]: the layer's FORWARD as TNR_DGRAD_4x4_S2 */
    TNR_PACK_UP2_FWD_S2D = 9   /* TNR_PACK_FWD_S2D's layout of S, [4][KoutP=ci][4*KinP=co]: its DATA-GRADIENT (the x2 sum included) as TNR_CONV_4x4_S2 */
};

#define TNR_MMA_F32 0
#define TNR_MMA_BF16 1
#define TNR_MMA_BF16X3 2

typedef struct tnr_view {
    float *ptr;
    int32_t ctot; /* channels per pixel of the underlying buffer */
    int32_t coff; /* first channel of this view                  */
} tnr_view;

/* One tiled implicit-GEMM convolution (forward, or data-gradient with dgrad-packed weights).
 * Replaces nn.Conv2d.forward + bias + (Leaky)ReLU(inplace) of block.conv_block (block.py:214-256),
 * the `x5*0.2 + x` / `out*0.2 + x` residuals (RRDBNet_arch.py:96,163), ShortcutBlock's add
 * (block.py:184-195), and in the backward direction aten::convolution_backward(input) with the
 * following leaky_relu_backward fused as a mask.
 *   v = act(acc + bias[c]);  v = v*alpha + (c < r1_ch ? beta1*r1[c] : 0);  if r2: v = v*alpha2 + r2[c];
 *   if m and m_lo <= c < m_hi:  v *= (m[c] > 0 ? 1 : m_slope);   y[c] = v                              */
typedef struct tnr_conv_desc {
    tnr_view x;            /* input activation (or incoming gradient for dgrad)               */
    int32_t N, H, W;       /* batch and SOURCE spatial size of x                               */
    int32_t Cin;           /* valid reduction channels in x                                    */
    const float *wp;       /* packed weights (tnr_pack_weights)                                */
    int32_t KinP, KoutP;   /* padded dims of the packing                                       */
    tnr_view y;            /* output                                                           */
    int32_t Ho, Wo, Cout;  /* output spatial size and channels stored                          */
    int32_t mode;          /* TNR_CONV_* */
    const float *bias;     /* [Cout] or NULL                                                   */
    int32_t act;           /* TNR_ACT_* applied to acc+bias                                    */
    float slope;
    float alpha;
    tnr_view r1; int32_t r1_ch; float beta1;   /* r1.ptr NULL = none */
    tnr_view r2; float alpha2;                 /* r2.ptr NULL = none */
    tnr_view m;  int32_t m_lo, m_hi; float m_slope; /* m.ptr NULL = none */
    /* optional split-K workspace (tnr_conv_workspace_bytes()).  A launch with too few output tiles to
     * fill the chip and a long reduction (the 512-channel layers at 16x16 and below) is split along K
     * into partial sums in ws, reduced in a fixed order by a second launch that applies bias / act / alpha.
     * NULL: never split.                                                                               */
    float *ws; int64_t ws_bytes;
    /* matrix-core operand precision: TNR_MMA_F32 = v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate: the default, bit
     * parity class of the CPU reference); TNR_MMA_BF16 = activations and weights rounded to bf16 (round-to-nearest-even) as
     * they enter the matrix core, v_mfma_f32_32x32x16_bf16, fp32 accumulate, fp32 epilogue and storage -- the engine's
     * `use_amp: true` policy (base_model.py:736-744 autocasts the convolutions to half precision);
     * TNR_MMA_BF16X3 = fp32 arithmetic on the bf16 matrix core: every operand is split EXACTLY into three bf16 values
     * (hi + mid + lo = x), the six largest of the nine partial products (each exact) are accumulated in fp32 -- the dropped
     * ones are below 2^-23 of the product by construction (2^-28 on average: less than fp32 rounding) -- at 6/16 of the fp32
     * matrix-core cycles.  Accepted by
     * tnr_conv_forward, tnr_conv_chain and tnr_wgrad / tnr_wgrad_group.  Finite inputs only: an infinite operand splits into
     * inf + NaN (the fp32 matrix core would deliver inf or NaN there as well); operands below 2^-110 lose their low split.  */
    int32_t mma;
    /* border handling of the TNR_CONV_3x3 mode: 0 = zero padding (nn.Conv2d padding 1), 1 = nn.ReflectionPad2d(1) in front of
     * an unpadded convolution (the ResnetGenerator's residual blocks, ResNet_arch.py:118-146): the stager reads row -1 as row 1
     * and row H as row H - 2, so the reflection-padded tensor is never materialised.                                      */
    int32_t pad_mode;
    /* ESRGAN+ GaussianNoise (block.py:587-600; ResidualDenseBlock_5C.forward RRDBNet_arch.py:160-163: `noise(x5*0.2 + x)`, on by
     * default, defaults.py:59): the epilogue value is multiplied by m = 1 + noise_sigma * n, n ~ N(0, 1), one draw per output element
     * -- `x + n * (sigma * x)` with the gradient through both terms, i.e. d/dx = m.  noise_pos: 0 none; 1 after the r1 step (forward:
     * v = (act(acc + bias) * alpha + beta1 r1) * m, then the r2 step: the RRDB residual sees the noised tensor); 2 after the r2 step
     * (backward: the gradient written by this launch enters a noised tensor).  n is never stored: it is a counter-based function of
     * (noise_key0, noise_key1, (noise_pix0 + output pixel) * Cout / 4 + channel / 4) -- see tnr_gauss_mult, which evaluates the same
     * function on a plain tensor -- so the backward pass regenerates the forward pass's draw bit for bit from the same key.
     * noise_pix0: first pixel of this rank's shard in the global batch (data-parallel ranks draw what one process would draw on the
     * concatenated batch).  Cout % 4 == 0; never combined with split-K; tnr_conv_sweep accepts it on the last stage only.          */
    float noise_sigma; int32_t noise_pos; uint32_t noise_key0, noise_key1, noise_pix0;
    /* optional: the layer's weights as a PRE-SPLIT stream (tnr_conv_wq_pack from the packed fp32 weights `wp`; valid until those
     * change) for TNR_MMA_BF16X3 / TNR_CONV_3x3 launches with Cout % 64 == 0 and Cin % 16 == 0: the kernel then takes its weight
     * fragments straight from L2 into registers (three bf16 planes in MFMA operand order, one coalesced 1 KB read per plane) instead
     * of splitting and staging the slab through LDS per workgroup and chunk.  NULL: the launch stages `wp` itself.  Same results
     * bit for bit either way.                                                                                                    */
    const void *wq; int64_t wq_bytes;
    /* which stream `wq` is: 0 = the tap-major one above (tnr_conv_wq_pack), 1 = the Winograd F(2x2, 3x3) transform-domain stream
     * (tnr_conv_wino_pack): the launch then runs as 16 transform-domain GEMMs per 2 x 2 output patch -- 2.25 x fewer matrix-core
     * instructions for the same convolution; the transforms cost a few extra fp32 roundings per element (error vs fp64 held to 3 x
     * the fp32 matrix core's in the tests, against 1.5 x for the direct forms) and the results are NOT bit-identical to them.      */
    int32_t wq_form;
    /* nn.PixelShuffle(2) behind the convolution (block.pixelshuffle_block, block.py:374-387: conv nf -> 4 nf, shuffle, act) folded into
     * the STORE: 0 = off; 2 = y is the SHUFFLED tensor [N, 2 Ho, 2 Wo, Cout / 4] and conv output channel 4 c + 2 dy + dx of pixel (oy, ox)
     * is written to channel c of pixel (2 oy + dy, 2 ox + dx) -- the [N, Ho, Wo, Cout] intermediate and the depth-to-space pass never
     * exist.  The epilogue (bias, act, alpha) is applied as usual (an elementwise activation commutes with the shuffle); residuals, mask
     * and noise are not supported.  Needs the pre-split weight stream (wq, wq_form = 0, built with this field set: the stream's cout
     * order follows the sub-pixel) and Cout % 256 == 0; anything else is refused -- the caller then runs tnr_depth_to_space itself.  */
    int32_t shuffle;
} tnr_conv_desc;

/* Weight-gradient of one convolution: dW[co][ci][ky][kx] = beta*dW + alpha * sum_pixels g * x
 * (aten::convolution_backward(weight, bias)), pixel-split into deterministic partial slabs in `ws`
 * and reduced in a fixed order.  The launch covers input channels [cin_begin, cin_begin+Cin) of a
 * layer whose weight tensor has cin_total input channels.                                        */
typedef struct tnr_wgrad_desc {
    tnr_view x; int32_t N, H, W; int32_t Cin;      /* layer input view (already offset to cin_begin) */
    tnr_view g; int32_t Ho, Wo; int32_t Cout;      /* gradient w.r.t. the conv output (pre-activation) */
    int32_t mode;                                  /* TNR_CONV_3x3 | _3x3_UP2 | _4x4_S2               */
    float *dw; int32_t cin_total, cin_begin;       /* OIHW gradient tensor                            */
    float *db;                                     /* [Cout] or NULL (only with cin_begin == 0)        */
    float alpha, beta;
    float *ws; int64_t ws_bytes;                   /* >= tnr_wgrad_workspace_bytes()                  */
    int32_t mma;                                   /* TNR_MMA_F32 | TNR_MMA_BF16 (see tnr_conv_desc)   */
    int32_t pad_mode;                              /* TNR_CONV_3x3: 0 zero padding, 1 reflection (tnr_conv_desc) */
    /* Two layers in one job ("cout pair"; cout_split = 0: off).  When the gradients of two layers that read the SAME input channels
     * stand side by side in one buffer -- a dense block's [g4 | g3] and [g2 | g1] (RRDBNet_arch.py:150-163) -- `g` may cover both
     * (Cout = 64): output channels [0, cout_split) then belong to the layer of dw / cin_total / db, channels [cout_split, Cout) to a
     * second layer dw2 / cin_total2 / db2 (same cin_begin, alpha, beta).  The pair runs in the 64-cout workgroup tile class: one
     * read of the input tile feeds both layers.  cout_split is a multiple of 32.                                               */
    float *dw2; int32_t cout_split, cin_total2;
    float *db2;
} tnr_wgrad_desc;

typedef struct tnr_pack_item {
    const float *w;  /* OIHW */
    float *wp;
    int32_t Cout, Cin, kh, kw;
    int32_t kind;    /* TNR_PACK_* */
    int32_t KoutP, KinP;
    int64_t n_out;   /* number of packed floats */
} tnr_pack_item;

/* "Gradient dense block": the data-gradient of a ResidualDenseBlock_5C (RRDBNet_arch.py:150-163) run as
 * the mirror image of its forward.  With the gradient buffer laid out [g5(nf) | g4 | g3 | g2 | g1]
 * (g_k = gradient w.r.t. conv_k's pre-activation output), the gradient w.r.t. the block's t-th feature
 * group (t = 0..4 -> x4, x3, x2, x1, x) is ONE convolution over the first nf + t*gc channels of that
 * buffer, with this packing of the transposed / flipped slices of W5..W(5-t) (conv5's slice pre-scaled by
 * scale5 = 0.2 * s).  No read-modify-write accumulation, K grows like in the forward pass.             */
typedef struct tnr_dense_pack_item {
    const float *w[5]; /* conv1..conv5 weights, OIHW */
    float *wp;
    int32_t nf, gc;
    int32_t t;         /* 0..4 */
    int32_t KoutP, KinP;
    float scale5;
    int64_t n_out;
} tnr_dense_pack_item;

const char *tnr_last_error(void);
/* ABI version = TNR_ABI_VERSION of the header the library was built from.  It moves whenever a descriptor struct changes size or
 * layout: a caller built against another header would pass a shorter struct and the library would read fields from adjacent memory.
 * Consumers compare it with THEIR header's TNR_ABI_VERSION before the first call (trainner_amd/hip.py does).
 *   1: rounds 1-4.   2: tnr_wgrad_desc gained dw2 / cout_split / cin_total2 / db2, TNR_WGRAD_GROUP_MAX 8 -> 12 (round 5; the number itself
 *      was bumped in round 6).   3: tnr_conv_desc gained wq_form and shuffle (round 6); tnr_wgrad_tile_class has since lost an argument: still 3. */
#define TNR_ABI_VERSION 3
int tnr_version(void);

/* --- convolution family ---------------------------------------------------------------------- */
int tnr_pack_dims(int32_t Cout, int32_t Cin, int32_t kh, int32_t kw, int32_t kind,
                  int32_t *KoutP, int32_t *KinP, int64_t *n_out);
/* items: DEVICE array of n descriptors; max_out = max n_out over the items */
int tnr_pack_weights(const tnr_pack_item *items_dev, int32_t n, int64_t max_out, void *stream);
/* The fold of the two TNR_PACK_UP2_* packings as a 16 x 9 matrix of 0 / 1 (host only, no launch): out[(ky*4 + kx)*9 + ty*3 + tx] = 1
 * where 3x3 tap (ty, tx) is summed into folded tap (ky, kx).  Its transpose takes the weight gradient of S back to the 3x3 taps:     */
int tnr_upconv_fold_table(int32_t out[144]);
/* dw3[co][ci][3][3] = beta*dw3 + alpha * unfold(dws[ci][co][4][4]): the weight gradient of a nearest-x2 3x3 layer from the weight
 * gradient of its folded S (tnr_conv_wgrad in TNR_CONV_4x4_S2 with x := gradient of the layer's output, g := the layer's input;
 * aten::convolution_backward(weight) of upconv_block's conv, block.py:326-371).  Per tap three fp32 additions in a fixed order
 * (inside a row of dws over ascending kx, then the two rows over ascending ky); one thread per (co, ci).  dws 16-byte aligned.        */
int tnr_upconv_wgrad_unfold(const float *dws, float *dw3, int32_t Cout, int32_t Cin, float alpha, float beta, void *stream);
int tnr_pack_dense_dims(int32_t nf, int32_t gc, int32_t t, int32_t *KoutP, int32_t *KinP, int64_t *n_out);
int tnr_pack_dense_dgrad(const tnr_dense_pack_item *items_dev, int32_t n, int64_t max_out, void *stream);
int tnr_conv_forward(const tnr_conv_desc *d, void *stream);
/* Host-only query (no device, no launch, no memory behind the descriptor's pointers is read): what tnr_conv_forward launches for the
 * descriptor AS IT STANDS -- wq / wq_form / ws / shuffle set or not --, through the code the entry itself decides by.  out[0] the kernel
 * (0 conv_tile, 1 conv3x3_x3w8, 2 conv3x3_d4, 3 conv_s2_d4, 4 conv3x3_wino); out[1..4] tw, th, nt (output channels per workgroup / 32),
 * mt (32-pixel M-tiles per wave; 0: the Winograd kernel has none); out[5..8] tiles_x, tiles_y, ncb, tiles (split-K: every split counted;
 * the stride-2 data-gradient: its four parity classes counted); out[9] ksplit; out[10] the persistent grid's cap in workgroups per CU
 * (the launch has min(tiles, cap x CUs) workgroups; 0: one workgroup per tile); out[11] 0.  A descriptor the entry refuses is refused
 * here with the same message (its check for null x / y / wp apart).                                   */
int tnr_conv_launch_class(const tnr_conv_desc *d, int32_t out[12]);
/* dst[p][c] = (src ? src[p][c] : 1) * (1 + sigma * n(key0, key1, (pix0 + p) * C / 4 + c / 4)) for `pixels` pixels of C channels: the
 * multiplier field of tnr_conv_desc.noise_* on a plain NHWC tensor (dst may alias src).  Used where the gradient of a noised tensor
 * is needed next to the plain one (the RRDB skip, RRDBNet_arch.py:96), and by tests to read the engine's draw.  C % 4 == 0.          */
int tnr_gauss_mult(tnr_view dst, tnr_view src, int64_t pixels, int32_t C, float sigma, uint32_t key0, uint32_t key1, uint32_t pix0,
                   void *stream);
int64_t tnr_conv_workspace_bytes(const tnr_conv_desc *d);   /* 0 when the launch would not be split */
/* size of / build the pre-split weight stream of a launch (tnr_conv_desc.wq); 0: the launch cannot use one */
int64_t tnr_conv_wq_bytes(const tnr_conv_desc *d);
int tnr_conv_wq_pack(const tnr_conv_desc *d, void *image, int64_t image_bytes, void *stream);
/* the same for the Winograd F(2x2, 3x3) form (tnr_conv_desc.wq with wq_form = 1): U = G g G^T of every (cout, cin) filter, computed in
 * fp64 from the packed fp32 weights, rounded once to fp32 and split into three bf16 planes in MFMA operand order.  64-cout blocks,
 * Cin % 16 == 0, TNR_MMA_BF16X3, stride 1, zero or reflection padding (nn.Conv2d k3 s1 p1, block.py:214-256; ResNet_arch.py:118-146). */
int64_t tnr_conv_wino_bytes(const tnr_conv_desc *d);
int tnr_conv_wino_pack(const tnr_conv_desc *d, void *image, int64_t image_bytes, void *stream);
/* nn.MaxPool2d(2, 2) behind the convolution's activation folded into the STORE of a Winograd-form launch, whose 2 x 2 output patch is the
 * pool window: d describes the unpooled launch (Ho = H, Wo = W, wq_form = 1) except that d->y is the POOLED tensor [N, Ho / 2, Wo / 2, Cout];
 * the full-resolution map never exists.  The stored value is bit for bit what tnr_maxpool2_fwd computes from the map tnr_conv_forward
 * would have stored (window scan order (0,0), (0,1), (1,0), (1,1), `v > best`: the first maximum wins).  route: NULL, or a dense
 * [N, Ho / 2, Wo / 2, Cout] byte map that receives per pooled element bits 0-1 = the arg-max position under that rule and bit 2 = "pooled
 * value > 0" -- everything tnr_maxpool2_bwd derives from the full-resolution map (tnr_unpool2_bwd takes the byte instead).
 * tnr_conv_pool_ok: 1 when the launch qualifies -- the Winograd form (tnr_conv_wino_bytes > 0), H and W even, ReLU or no activation, no
 * r1 / r2 / mask / noise / shuffle / split-K workspace --, else 0: the caller then runs tnr_conv_forward and tnr_maxpool2_fwd.
 * The request travels as arguments of an entry of its own, not as descriptor members: tnr_conv_desc keeps its layout (ABI 3).          */
int tnr_conv_pool_ok(const tnr_conv_desc *d);
int tnr_conv_forward_pool2(const tnr_conv_desc *d, uint8_t *route, void *stream);
/* out[(n*Ho + oy)*Wo + ox][(ky*kw + kx)*C + c] = x[n][oy*stride - pad + ky][ox*stride - pad + kx][c] (0 outside):
 * the patch matrix of a k x k convolution as an NHWC "image" of Ho*Wo*N pixels with kh*kw*C channels, for
 * TNR_CONV_1x1 with TNR_PACK_COL_* weights.  C % 4 == 0.                                                */
int tnr_im2col(tnr_view x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride, int32_t pad,
               int32_t Ho, int32_t Wo, float *out, void *stream);
/* n <= TNR_CHAIN_MAX dependent 3x3 convolutions over one pixel grid in ONE launch: the five convolutions of a
 * ResidualDenseBlock_5C (RRDBNet_arch.py:150-163) or of its gradient mirror.  Stage i may read what stages
 * < i of the same call wrote: fresh_from[i] is the first input channel of stage i that stage i-1 produced
 * (-1: none; channels below it must predate the call or come from stages <= i-2).  A workgroup keeps its
 * 16x32-pixel tile through all stages and waits, at that channel, for the 8 neighbouring tiles (3x3 halo)
 * through per-tile progress counters in ws (tnr_conv_chain_workspace_bytes(), zeroed once; the last word
 * becomes nonzero if a wait ever gave up).  epoch must grow by 1 per call on the same ws.  Every stage:
 * mode TNR_CONV_3x3, same N/H/W, Cout % 32 == 0, KoutP == Cout; epilogues as in tnr_conv_forward.  Outputs of
 * different stages must not overlap, and no stage may write channels another stage of the call reads
 * before its fresh_from point.  Results are bit-identical to n tnr_conv_forward calls.                    */
#define TNR_CHAIN_MAX 6
int64_t tnr_conv_chain_workspace_bytes(const tnr_conv_desc *stage0);
int tnr_conv_chain(const tnr_conv_desc *stages, const int32_t *fresh_from, int32_t n, uint32_t *ws, int64_t ws_bytes,
                   uint32_t epoch, void *stream);
/* The same five convolutions of a residual dense block (RRDBNet_arch.py:150-163: stage k reads channels [0, nf + 32 k) of ONE buffer
 * and, except the last, writes the next 32 channels of it; 32, 32, 32, 32, 64 output channels) -- or of its gradient mirror -- as a
 * SWEEP: TNR_MMA_BF16X3 only.  One workgroup keeps the accumulators of all 192 output channels of its 8 x 32 pixel tile in
 * registers and reads every input channel chunk once per phase for all the stages that consume it, with the weights streamed
 * pre-split (three bf16 planes) from `image`, which tnr_conv_sweep_pack builds from the stages' packed fp32 weights (d->wp) and
 * which stays valid until those change.  tnr_conv_sweep_image_bytes returns 0 when the stages are not such a block (or an
 * image's tiles exceed the co-resident workgroups): use tnr_conv_chain then.  ws / epoch as for tnr_conv_chain (same buffer,
 * same counter; the buffer also holds the launch's tile dispenser, which every launch leaves at zero: one launch at a time per ws,
 * i.e. one ws per stream).  Results are bit-identical to tnr_conv_chain / five tnr_conv_forward calls in TNR_MMA_BF16X3.
 * n = 4 (TNR_MMA_BF16X3 only): the first four stages of such a block -- 32 output channels each --
 * with an image of their own; bit-identical to four tnr_conv_forward calls.                                                 */
int64_t tnr_conv_sweep_image_bytes(const tnr_conv_desc *stages, int32_t n);
int tnr_conv_sweep_pack(const tnr_conv_desc *stages, int32_t n, void *image, int64_t image_bytes, void *stream);
int tnr_conv_sweep(const tnr_conv_desc *stages, int32_t n, const void *image, uint32_t *ws, int64_t ws_bytes, uint32_t epoch,
                   void *stream);
/* 3x3 s1 p1 convolution with Cout <= 4 on the vector ALUs (one thread = one pixel x 4 outputs): G's last conv
 * (RRDBNet_arch.py:44) and the data-gradients that end in the RGB image (VGG features[0], D's first conv).
 * y[c] = (sum + bias[c]) * alpha for c < Cout.  Weights: tnr_conv_thin_pack (dgrad = 0: forward of a layer with
 * Cout <= 4; dgrad = 1: data-gradient of a layer with Cin <= 4, then Cin/Cout of tnr_conv_thin are the layer's
 * Cout/Cin) into tnr_conv_thin_pack_floats(reduction channels) floats.                                     */
int64_t tnr_conv_thin_pack_floats(int32_t reduce_channels);
int tnr_conv_thin_pack(const float *w_oihw, float *wp, int32_t Cout, int32_t Cin, int32_t dgrad, void *stream);
int tnr_conv_thin(tnr_view x, int32_t N, int32_t H, int32_t W, int32_t Cin, const float *wp, tnr_view y, int32_t Cout,
                  const float *bias, float alpha, void *stream);
/* The same for the 7x7 image-side layers of ResnetGenerator (ResNet_arch.py:52-55, :86-88), one launch for the 49 taps:
 *   y[n, oy, ox, c] = (sum_{t, ci} w[t][ci][c] * x[n, oy + ty - pad, ox + tx - pad, ci] + bias[c]) * alpha   (c < Cout <= 4)
 * over an Ho x Wo output grid; reflect = 1: ReflectionPad2d(pad) borders (pad <= 3, Ho x Wo = H x W), reflect = 0: zeros outside
 * the H x W input -- with pad = 6 and Ho x Wo = (H + 6) x (W + 6) that is the data-gradient of a 7x7 layer with respect to its
 * reflection-padded input (fold it back with tnr_unpad2d).  Weights: tnr_conv_thin7_pack (dgrad as in tnr_conv_thin_pack) into
 * tnr_conv_thin7_pack_floats(reduction channels) floats.  Cout <= 3 and Cin <= 64 run with one lane per INPUT channel (weights in
 * registers, coalesced input rows, per-pixel sums through LDS); a 4-channel output or more input channels with one lane per pixel.  */
int64_t tnr_conv_thin7_pack_floats(int32_t reduce_channels);
int tnr_conv_thin7_pack(const float *w_oihw, float *wp, int32_t Cout, int32_t Cin, int32_t dgrad, void *stream);
int tnr_conv_thin7(tnr_view x, int32_t N, int32_t H, int32_t W, int32_t Cin, const float *wp, tnr_view y, int32_t Ho, int32_t Wo,
                   int32_t Cout, int32_t pad, int32_t reflect, const float *bias, float alpha, void *stream);
int64_t tnr_wgrad_workspace_bytes(const tnr_wgrad_desc *d);
/* Weight (+ bias) gradient of a 3x3 s1 p1 layer with <= 3 channels on one side, on the vector ALUs:
 * flip = 0: a Csmall -> Cbig layer (big = gradient of its output, small = its NHWC4 input image),
 *           dw = [Cbig][Csmall][3][3], db = [Cbig];
 * flip = 1: a Cbig -> Csmall layer (big = its input, small = NHWC4 gradient of its output),
 *           dw = [Csmall][Cbig][3][3], db = [Csmall].
 * dw = beta*dw + alpha*sum (db likewise, may be NULL).  Cbig in {16, 32, 64}.  Deterministic.               */
int64_t tnr_wgrad_thin_workspace_bytes(int32_t N, int32_t H, int32_t Cbig);
int tnr_wgrad_thin(tnr_view big, tnr_view small, int32_t N, int32_t H, int32_t W, int32_t Cbig, int32_t Csmall, int32_t flip,
                   float *dw, float *db, float alpha, float beta, float *ws, int64_t ws_bytes, void *stream);
/* The same for a 7x7 layer, one launch for the 49 taps (+ one reduce launch):
 *   acc[cb][cs][ty][tx] = sum over the big grid q of big(q)[cb] * small[q + (ty, tx) + off][cs]      (small: zeros outside Hs x Ws)
 * big grid = (H + 2 rpad) x (W + 2 rpad), big(q) = the H x W buffer at the ReflectionPad2d(rpad) image of q (rpad = 0: the buffer).
 * flip = 0: dw[cb][cs][t] = acc[..][t]       -- an image -> Cbig layer: big = gradient of its output, small = its reflection-padded
 *           NHWC4 input image ((H + 6) x (W + 6)), off = 0; db[cb] = sum of big (may be NULL);
 * flip = 1: dw[cs][cb][t] = acc[..][48 - t]  -- a Cbig -> image layer: big = its input read through ReflectionPad2d(3) (rpad = 3),
 *           small = the NHWC4 gradient of its output (H x W), off = -6; db must be NULL (sum the 4-channel gradient elsewhere).
 * dw = beta*dw + alpha*acc.  Cbig in {16, 32, 64}, Csmall <= 3.  Deterministic.                               */
int64_t tnr_wgrad_thin7_workspace_bytes(int32_t N, int32_t Hbig_grid, int32_t Cbig);
int tnr_wgrad_thin7(tnr_view big, int32_t N, int32_t H, int32_t W, int32_t rpad, tnr_view small, int32_t Hs, int32_t Ws, int32_t off,
                    int32_t Cbig, int32_t Csmall, int32_t flip, float *dw, float *db, float alpha, float beta, float *ws, int64_t ws_bytes,
                    void *stream);
int tnr_conv_wgrad(const tnr_wgrad_desc *d, void *stream);
/* n <= TNR_WGRAD_GROUP_MAX layers in ONE launch (+ one reduce launch).  The layers must share mode and
 * N/H/W/Ho/Wo and fall into the same workgroup tile class (same Cout <= 32 | > 32 and the same number of
 * 32-channel input blocks per workgroup: e.g. the 64-input pieces of a dense block's conv1/conv3/conv4);
 * each needs its own workspace of tnr_wgrad_workspace_bytes().  Results equal n single launches up to
 * the summation order of the split-K partials (still run-to-run deterministic).                     */
#define TNR_WGRAD_GROUP_MAX 12
int tnr_conv_wgrad_group(const tnr_wgrad_desc *descs, int32_t n, void *stream);
/* Host-only query, no device and no launch: the workgroup tile class tnr_conv_wgrad_group runs `d` on when its launch carries group_jobs
 * (cin block, cout block) jobs (0: the layer alone).  out = {mode, A_T, B_T, THG, BF, WPS, DB (the kernel's template arguments), KS, splits,
 * tiles_per_split, LDS bytes, index in the library's class table}.  Reads d's shape fields, mode, mma, pad_mode, the views' ctot.  TNR_EINVAL: no kernel. */
int tnr_wgrad_tile_class(const tnr_wgrad_desc *d, int32_t group_jobs, int32_t out[12]);

/* --- image-to-image family (Pix2Pix / CycleGAN: ResnetGenerator ResNet_arch.py:11-90, NLayerDiscriminator
 * discriminators.py:472-579).  Generic convolution on the vector ALUs for the layers outside the matrix-core geometries
 * (7x7 reflection-padded first / last convolutions, the PatchGAN's 4x4 stride-1 layers): any square kernel k, stride,
 * zero (reflect = 0) or nn.ReflectionPad2d (reflect = 1, stride 1) padding; OIHW weights as stored in the state_dict.
 *   fwd:   y = act(conv(x, w) + bias);  dgrad: gx = conv_backward_data(g, w) (reflection folded back);
 *   wgrad: dw = beta dw + alpha sum g (x) x, db likewise (db may be NULL); two-stage fp64 reduction in a fixed order,
 *          ws: tnr_gconv_wgrad_workspace_bytes(Cout, Cin, k).
 * tnr_pad2d / tnr_unpad2d: materialise a zero (mode 0) or reflection (mode 1) border of `pad` pixels / crop it (mode 0) or
 * apply the adjoint of the reflection padding (mode 1) -- the residual blocks' reflection-padded 3x3 convolutions run on
 * the MFMA 3x3 kernel over the padded tensor.  tnr_tanh_*: the generator's output activation.  tnr_gan_loss: GANLoss
 * against a constant label (modules/loss.py:61-137): type 0 vanilla (BCE with logits), 1 lsgan (MSE), mean reduction,
 * 2 = mean(pred) (the D_real / D_fake log entries, losses.py:519-520); out[0] = loss, grad = d loss / d pred (may be NULL). */
int tnr_gconv_fwd(tnr_view x, int32_t N, int32_t H, int32_t W, int32_t Cin, const float *w, const float *bias, tnr_view y, int32_t Ho,
                  int32_t Wo, int32_t Cout, int32_t k, int32_t stride, int32_t pad, int32_t reflect, int32_t act, float slope, void *stream);
int tnr_gconv_dgrad(tnr_view g, int32_t N, int32_t H, int32_t W, int32_t Cin, const float *w, tnr_view gx, int32_t Ho, int32_t Wo,
                    int32_t Cout, int32_t k, int32_t stride, int32_t pad, int32_t reflect, void *stream);
int64_t tnr_gconv_wgrad_workspace_bytes(int32_t Cout, int32_t Cin, int32_t k);
int tnr_gconv_wgrad(tnr_view x, int32_t N, int32_t H, int32_t W, int32_t Cin, tnr_view g, int32_t Ho, int32_t Wo, int32_t Cout, int32_t k,
                    int32_t stride, int32_t pad, int32_t reflect, float *dw, float *db, float alpha, float beta, double *ws,
                    int64_t ws_bytes, void *stream);
/* db = beta db + alpha sum_pixels g[p][c] (bias gradient of a layer whose weight gradient runs on another kernel);
 * ws: >= 512 * C doubles (two-stage column sum in a fixed order; >= 64 * C selects the slow generic path).          */
int tnr_bias_grad(tnr_view g, int64_t pixels, int32_t C, float *db, float alpha, float beta, double *ws, int64_t ws_bytes, void *stream);
int tnr_pad2d(tnr_view x, tnr_view y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t pad, int32_t mode, void *stream);
int tnr_unpad2d(tnr_view xp, tnr_view y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t pad, int32_t mode, void *stream);
/* dst[n,y,x,:] (+)= src[n, y+oy, x+ox, :] inside the source, 0 outside (zero-embedding at an offset / offset crop; acc != 0
 * adds to dst): kernel geometries without their own tile run as shifted 3x3 windows of the 3x3 kernels -- the PatchGAN's 4x4
 * stride-1 layers (discriminators.py:543-560: weight gradient = four windows) and the ResnetGenerator's 7x7 reflection-padded
 * first / last convolutions (ResNet_arch.py:52-55,86-88: nine 3x3 blocks of taps).                                      */
int tnr_window2d(tnr_view src, int32_t Hs, int32_t Ws, tnr_view dst, int32_t N, int32_t Hd, int32_t Wd, int32_t C, int32_t oy,
                 int32_t ox, int32_t acc, void *stream);
int tnr_tanh_fwd(const float *x, float *y, int64_t n, void *stream);
int tnr_tanh_bwd(const float *g, const float *y, float *gx, int64_t n, void *stream);
int tnr_gan_loss(const float *pred, int64_t n, int32_t type, float target, float *out, float *grad, void *stream);
/* --- data-parallel collectives (RCCL over xGMI; replaces nn.DataParallel's reduce_add of replica gradients,
 * networks.py:252-255).  One communicator per process.  Rank 0 fills a 128-byte id with tnr_dp_unique_id and shares it
 * out of band; every rank calls tnr_dp_init(id, rank, world, &comm).  Per optimiser step: tnr_dp_allreduce_bucket(comm,
 * bucket, count, average = 1, side_stream) for every gradient bucket as soon as its last gradient kernel is enqueued
 * (in place; ncclAvg = mean over ranks), tnr_dp_broadcast to align replicas at start, tnr_dp_finalize at exit.
 * librccl is dlopen()ed on first use.  Calls on one communicator must be issued in the same order on every rank.     */
int tnr_dp_unique_id(void *id128);
int tnr_dp_init(const void *id128, int32_t rank, int32_t world, void **comm);
int tnr_dp_allreduce_bucket(void *comm, float *buf, int64_t count, int32_t average, void *stream);
int tnr_dp_broadcast(void *comm, float *buf, int64_t count, int32_t root, void *stream);
/* the communicator's own rank count (ncclCommCount): what bench.py reports as config.world_size_observed */
int tnr_dp_comm_count(void *comm, int32_t *nranks);
int tnr_dp_finalize(void *comm);
/* Real-ESRGAN style degradations on fp32 NCHW images in [0, 1] (the LR synthesis the reference runs per sample with
 * OpenCV on DataLoader workers: dataops/augmentations.py:1666-1801, options/presets/resrgan_*.yaml).
 * tnr_filter2d: cv2.filter2D semantics (correlation, centred anchor, BORDER_REFLECT_101) with one 21 x 21 kernel slot per
 *   image (smaller kernels centred, zeros around) -- iso / aniso Gaussian and sinc blurs of 7..21 taps.
 * tnr_resize: cv2.resize semantics for mode 0 INTER_AREA, 1 INTER_LINEAR, 2 INTER_CUBIC on NC planes of H x W -> Ho x Wo.
 * tnr_noise_gaussian: x += sigma255[n][c] / 255 * N(0, 1) (grey[n]: one draw per pixel for all channels, sigma255[n][0]).
 * tnr_noise_poisson: x += scale[n] * (Poisson(x * vals[n]) / vals[n] - x), the difference reduced to luma when grey[n].
 *   Both in place, counter-based RNG (Philox4x32-10 keyed by seed and sample): reproducible for a given seed.
 * tnr_jpeg_sim: in place JPEG round trip of RGB images at quality[n] (JFIF YCbCr, 4:2:0, 8x8 DCT, Annex-K tables with
 *   libjpeg's quality scaling, triangle chroma up-sampling); ws: tnr_jpeg_workspace_bytes(N, H, W).            */
int tnr_filter2d(const float *src, float *dst, const float *kernels21, int32_t N, int32_t C, int32_t H, int32_t W, void *stream);
int tnr_resize(const float *src, float *dst, int32_t NC, int32_t H, int32_t W, int32_t Ho, int32_t Wo, int32_t mode, void *stream);
int tnr_noise_gaussian(float *img, int32_t N, int32_t C, int32_t H, int32_t W, const float *sigma255, const int32_t *grey,
                       uint64_t seed, int32_t clip, void *stream);
int tnr_noise_poisson(float *img, int32_t N, int32_t C, int32_t H, int32_t W, const float *vals, const float *scale,
                      const int32_t *grey, uint64_t seed, int32_t clip, void *stream);
int64_t tnr_jpeg_workspace_bytes(int32_t N, int32_t H, int32_t W);
int tnr_jpeg_sim(float *img, int32_t N, int32_t H, int32_t W, const int32_t *quality, float *ws, int64_t ws_bytes, void *stream);
/* Input feed (wire format: uint8 HWC BGR crop windows, as OpenCV hands the reference's datasets): one launch per batch
 * does the paired flip / rot90 of dataops/augmentations.py:790-830 and np2tensor of dataops/common.py:470-499
 * (x * data_range / 255, HWC -> CHW, BGR(A) -> RGB(A), optional norm()).  src [N,H,W,C] uint8 (device), dst
 * [N,C,H,W] float; flags[n] (device int32, may be NULL): bit 0 flip (np.flip axis 1), bit 1 rot (np.rot90 k = 1),
 * bit 2 vflip (np.flip axis 0 before the rotation; only with rot).  any_rot != 0 requires H == W.            */
int tnr_feed_u8_to_tensor(const uint8_t *src, int32_t N, int32_t H, int32_t W, int32_t C, const int32_t *flags, int32_t any_rot,
                          float *dst, int32_t bgr2rgb, float data_range, int32_t normalize, void *stream);
/* Validation metrics on the device (the reference does these on the host: tensor2np dataops/common.py:502-566,
 * calculate_psnr / calculate_ssim utils/metrics.py:110-126,180-223, driven by train.py:335-372).
 * tnr_tensor2np_u8: NCHW float -> NHWC uint8 = round_half_even(clip(255 * x, 0, 255)), x -> (x + 1) / 2 first if
 *   denormalize, channels RGB(A) -> BGR(A) if rgb2bgr (every image of the batch; the reference keeps image 0).
 * tnr_psnr_ssim_u8: per image n, out[4n .. 4n+3] = {sum of squared differences, element count, sum of the SSIM map,
 *   SSIM map element count} over the images cropped by `crop` border pixels (SSIM: 11x11 Gaussian window sigma 1.5,
 *   'valid' region, fp64; count 0 if the cropped image is smaller than the window or want_ssim == 0).
 *   PSNR = 20 log10(255 / sqrt(sum / count)); SSIM = sum / count.  ws: tnr_metrics_workspace_bytes(N).           */
int tnr_tensor2np_u8(const float *src, int32_t N, int32_t C, int32_t H, int32_t W, uint8_t *dst, int32_t rgb2bgr,
                     int32_t denormalize, void *stream);
int64_t tnr_metrics_workspace_bytes(int32_t N);
int tnr_psnr_ssim_u8(const uint8_t *a, const uint8_t *b, int32_t N, int32_t H, int32_t W, int32_t C, int32_t crop,
                     int32_t want_ssim, double *out, double *ws, int64_t ws_bytes, void *stream);
/* LPIPS validation metric, net-lin / squeeze / v0.1 / spatial = False (utils/metrics.py:37,232-280 ->
 * models/modules/LPIPS/networks_basic.py:32-120).  The Fire convolutions of the SqueezeNet 1.1 backbone are tnr_conv_forward launches.
 * tnr_lpips_stem: ScalingLayer + features[0] (conv 3x3 stride 2 no padding, 3 -> 64, bias) + ReLU of the image pairs (a[n], b[n]):
 *   y = relu1 of the 2N images [a[0..N-1], b[0..N-1]], NHWC [2N, Ho, Wo, 64] (tnr_lpips_stem_dims).  src_kind 0: uint8 NHWC
 *   [N, H, W, 3] (x = u8 / 127.5 - 1, divided in fp64, rounded to fp32), cropped by `crop` pixels per side; src_kind 1: fp32
 *   NCHW [N, 3, H, W] in [-1, 1] (x = 2 x - 1 first if normalize).  shift / scale: the ScalingLayer buffers (3 floats each);
 *   w: the OIHW [64, 3, 3, 3] weight, bias [64].
 * tnr_maxpool3s2_ceil_fwd: nn.MaxPool2d(3, stride 2, ceil_mode = True), output size per tnr_maxpool3s2_ceil_dims; C % 4 == 0.
 * tnr_lpips_head: per image n, the fixed-order fp64 sum over pixels of sum_c w[c] (f0[c] / (|f0| + 1e-10) - f1[c] / (|f1| + 1e-10))^2,
 *   f0 / f1 = image n of the two views, into layer `layer` (of L) of ws (tnr_lpips_workspace_bytes(N, L)).
 * tnr_lpips_finalize: out[n] (fp64) = sum over the L layers of the layer's sum / its pixel count; per_layer (optional, [N, L])
 *   receives the terms.  Deterministic: bit-identical across runs; exactly 0 for identical features.                            */
int tnr_lpips_stem_dims(int32_t H, int32_t W, int32_t crop, int32_t *Ho, int32_t *Wo);
int tnr_lpips_stem(const void *a, const void *b, int32_t src_kind, int32_t N, int32_t H, int32_t W, int32_t C, int32_t crop,
                   int32_t normalize, const float *shift, const float *scale, const float *w, const float *bias, tnr_view y,
                   void *stream);
int tnr_maxpool3s2_ceil_dims(int32_t H, int32_t W, int32_t *Ho, int32_t *Wo);
int tnr_maxpool3s2_ceil_fwd(tnr_view x, tnr_view y, int32_t N, int32_t H, int32_t W, int32_t C, void *stream);
int64_t tnr_lpips_workspace_bytes(int32_t N, int32_t L);
int tnr_lpips_head(tnr_view f0, tnr_view f1, int32_t N, int32_t H, int32_t W, int32_t C, const float *w, int32_t layer, int32_t L,
                   double *ws, int64_t ws_bytes, void *stream);
int tnr_lpips_finalize(int32_t N, int32_t L, const double *ws, int64_t ws_bytes, double *out, double *per_layer, void *stream);
/* Bilinear x2 up-sampling, align_corners = False, and its adjoint -- F.interpolate(x, scale_factor=2, mode='bilinear',
 * align_corners=False) between the decoder convolutions of UNetDiscriminator (discriminators.py:745-769).
 * fwd: x [N,H,W,C] -> y [N,2H,2W,C].  bwd: gy [N,2H,2W,C] -> gx (plain, may be null) and / or
 * gz = gx * LeakyReLU'(mask) (may be null; mask is the activation whose sign gates: > 0 -> 1, else mslope).   */
int tnr_bilinear2x_fwd(tnr_view x, tnr_view y, int32_t N, int32_t H, int32_t W, int32_t C, void *stream);
int tnr_bilinear2x_bwd(tnr_view gy, tnr_view gx, tnr_view gz, tnr_view mask, float mslope, int32_t N, int32_t H, int32_t W,
                       int32_t C, void *stream);
/* dst = a + b over `pixels` x C (the U-Net skip connections x4 + x2, x5 + x1, x6 + x0: discriminators.py:755,762,769);
 * dst = src * LeakyReLU'(y) out of place (src stays intact for the skip path of the backward pass).          */
int tnr_add2(tnr_view dst, tnr_view a, tnr_view b, int64_t pixels, int32_t C, void *stream);
int tnr_mask_copy(tnr_view dst, tnr_view src, tnr_view y, int64_t pixels, int32_t C, float mslope, void *stream);
/* --- layout / resampling (block.py:326-371 Upsample, :374-387,434-460 PixelShuffle; nn.MaxPool2d) */
int tnr_nchw_to_nhwc(const float *src, int32_t N, int32_t C, int32_t H, int32_t W, tnr_view dst,
                     int32_t Cpad, const float *scale, const float *shift, void *stream);
int tnr_nhwc_to_nchw(tnr_view src, int32_t N, int32_t C, int32_t H, int32_t W, float *dst,
                     const float *scale, int32_t accumulate, void *stream);
int tnr_upsample2x_bwd(tnr_view gup, tnr_view gx, int32_t N, int32_t H, int32_t W, int32_t C,
                       tnr_view mask, float mslope, void *stream);
int tnr_depth_to_space(tnr_view x, tnr_view y, int32_t N, int32_t H, int32_t W, int32_t Cout, void *stream);
int tnr_space_to_depth_bwd(tnr_view gy, tnr_view gx, int32_t N, int32_t H, int32_t W, int32_t Cout,
                           tnr_view mask, float mslope, void *stream);
int tnr_maxpool2_fwd(tnr_view x, tnr_view y, int32_t N, int32_t H, int32_t W, int32_t C, void *stream);
int tnr_maxpool2_bwd(tnr_view gy, tnr_view x, tnr_view gx, int32_t N, int32_t H, int32_t W, int32_t C,
                     void *stream);
/* tnr_maxpool2_bwd from the byte map of tnr_conv_forward_pool2 instead of the full-resolution activation: gx[N, H, W, C] gets gy[N, H / 2,
 * W / 2, C] at the window position in bits 0-1 of the element's byte when bit 2 is set, zeros everywhere else (bit-identical to
 * tnr_maxpool2_bwd on the map the unfused launch stores).  map: dense [N, H / 2, W / 2, C] bytes, 4-byte aligned.                       */
int tnr_unpool2_bwd(tnr_view gy, const uint8_t *map, tnr_view gx, int32_t N, int32_t H, int32_t W, int32_t C, void *stream);
int tnr_axpby(tnr_view dst, tnr_view src, int64_t pixels, int32_t C, float a, float b, void *stream);
int tnr_mask_mul(tnr_view g, tnr_view y, int64_t pixels, int32_t C, float mslope, void *stream);
int tnr_fill(float *p, int64_t n, float v, void *stream);

/* --- BatchNorm2d training mode (nn.BatchNorm2d via block.norm, block.py:112-134) + LeakyReLU ---- */
int64_t tnr_bn_workspace_bytes(int32_t C);
int tnr_bn_train_fwd(tnr_view z, tnr_view y, int64_t pixels, int32_t C, const float *gamma,
                     const float *beta, float *running_mean, float *running_var, int64_t *num_batches,
                     float momentum, float eps, float *save_mean, float *save_invstd, int32_t act,
                     float slope, void *ws, void *stream);
/* tnr_bn_train_fwd that also records, in stat64[2 C] (fp64: batch mean, unbiased variance; may be NULL), the exact values of its
 * running-statistics update, and tnr_bn_replay_running, which applies that update (and the batch counter increment) once more:
 * the side effects of a second training-mode forward over the same batch with the same parameters.  The SR step shows the
 * discriminator the real and the fake batch twice (generator stage sr_model.py:170-177 -> losses.py:398-403; discriminator stage
 * :190-193 -> losses.py:471-478) between two discriminator updates: the engine keeps the first pass's activations and replays
 * only these side effects instead of recomputing an identical forward (models/sr_model.py, HipNet.memoize).               */
int tnr_bn_train_fwd_stats(tnr_view z, tnr_view y, int64_t pixels, int32_t C, const float *gamma, const float *beta,
                           float *running_mean, float *running_var, int64_t *num_batches, float momentum, float eps,
                           float *save_mean, float *save_invstd, double *stat64, int32_t act, float slope, void *ws, void *stream);
int tnr_bn_replay_running(float *running_mean, float *running_var, int64_t *num_batches, const double *stat64, int32_t C,
                          float momentum, void *stream);
int tnr_bn_train_bwd(tnr_view gy, tnr_view y, tnr_view z, tnr_view gz, int64_t pixels, int32_t C,
                     const float *gamma, const float *save_mean, const float *save_invstd, float mslope,
                     float *dgamma, float *dbeta, float acc_beta, void *ws, void *stream);
/* The same with the LeakyReLU / ReLU mask RECOMPUTED from z instead of read from y: y > 0 <=> ((z - mean) invstd) gamma + beta > 0 is
 * the forward's own expression (tnr_bn_train_fwd; the library is built with -ffp-contract=off), so the mask -- and every result -- is
 * bit-for-bit that of tnr_bn_train_bwd; one of the two passes' three reads per element disappears.  gamma / beta must be the
 * values the forward ran with (true between a forward and its backward).                                                       */
int tnr_bn_train_bwd_z(tnr_view gy, tnr_view z, tnr_view gz, int64_t pixels, int32_t C, const float *gamma, const float *beta,
                       const float *save_mean, const float *save_invstd, float mslope, float *dgamma, float *dbeta,
                       float acc_beta, void *ws, void *stream);
/* InstanceNorm2d without affine parameters or running statistics (the ResnetGenerator's norm layer, ResNet_arch.py:40-50 ->
 * nn.InstanceNorm2d defaults) over a whole batch: the BatchNorm kernels with one statistics group per image.
 * y = act((z - mean[n,c]) * invstd[n,c]); save_mean / save_invstd: [N * C].  bwd: gz from gy (masked by act'(y), slope mslope:
 * 0 ReLU, 1 none).  ws: tnr_instnorm_workspace_bytes(N, C).                                                            */
int64_t tnr_instnorm_workspace_bytes(int32_t N, int32_t C);
int tnr_instnorm_fwd(tnr_view z, tnr_view y, int32_t N, int64_t pixels_per_image, int32_t C, float eps, float *save_mean,
                     float *save_invstd, int32_t act, float slope, void *ws, void *stream);
int tnr_instnorm_bwd(tnr_view gy, tnr_view y, tnr_view z, tnr_view gz, int32_t N, int64_t pixels_per_image, int32_t C,
                     const float *save_mean, const float *save_invstd, float mslope, void *ws, void *stream);

/* --- classifier (nn.Linear, discriminators.py:40-45) ------------------------------------------- */
int tnr_linear_fwd(const float *x, const float *w, const float *b, float *y, int32_t N, int32_t In,
                   int32_t Out, int32_t act, float slope, void *stream);
int tnr_linear_bwd(const float *x, const float *w, const float *gy, const float *yact, float mslope,
                   float *gx, float *dw, float *db, int32_t N, int32_t In, int32_t Out, float acc_beta,
                   float *gpre_ws, void *stream);

/* --- losses (nn.L1Loss losses.py:37-39; GANLoss loss.py:61-137; Adversarial losses.py:428-433,503-512) */
int64_t tnr_reduce_workspace_bytes(void);
int tnr_l1_mean_fwd(const float *a, const float *b, int64_t n, float scale, float *loss, void *ws,
                    void *stream);
int tnr_l1_mean_bwd(const float *a, const float *b, int64_t n, float scale, const float *gscale,
                    float *ga, int32_t accumulate, void *stream);
/* relativistic BCE, three phases so that the two 2-scalar sums can be all-reduced between them
 * (SURVEY.md 8(e)); sums = 8 floats on device.  stage 0 = generator, 1 = discriminator.
 * ws: tnr_reduce_workspace_bytes() of scratch for the two-stage (fixed-order) reductions over per-pixel logit maps (n >= 4096:
 * UNetDiscriminator); NULL or smaller n: one block reduces everything.                                                      */
int tnr_ragan_phase_a(const float *pf, const float *pr, int32_t n, float *sums, void *ws, void *stream);
int tnr_ragan_phase_b(const float *pf, const float *pr, int32_t n, int32_t stage, float *sums, void *ws, void *stream);
int tnr_ragan_phase_c(const float *pf, const float *pr, int32_t n, int32_t stage, float weight,
                      const float *sums, float *loss_out, float *gf, float *gr, void *stream);
int tnr_scale_by(float *dst, const float *src, int64_t n, const float *gscale, void *stream);

/* --- SSIM / MS-SSIM training losses (modules/ssim.py; get_loss_fn losses.py:70-85) --------------
 * fp32 image batches x (carries the gradient) and y, N x C x H x W with 1..4 channels, layout 0 = NCHW-contiguous, 1 = channels-last.
 * `shave` pixels are cut off every side first (their gradient is 0).  taps: K window taps on the HOST (K odd, <= 11), applied as a
 * row pass then a column pass without padding, so the maps are (H - 2 shave - K + 1) x (W - 2 shave - K + 1).
 * tnr_ssim_fwd: sums[n] = {sum ssim_map, sum cs_map} of image n over its C planes, fp64, fixed order (ws: tnr_ssim_workspace_bytes).
 * tnr_ssim_bwd: gx (x's shape and layout; written, or added into when `accumulate`) = gscale[0] * sum over the maps of
 *   coef[n][0] * d ssim_map / dx + coef[n][1] * d cs_map / dx; coef ([N][2]) and gscale (1 float, NULL = 1) are read on the device.
 *   The moments are recomputed from x and y; sigma1_sq / sigma2_sq are clamped at 0 as ssim.py:181-182 (no gradient through a
 *   clamped sigma1_sq).  y gets no gradient.
 * tnr_avgpool2_pad_fwd: F.avg_pool2d(kernel 2, padding (h % 2, w % 2), count_include_pad) of the shaved x and y -> xo, yo, dense
 *   NCHW [N, C, Ho, Wo] (tnr_avgpool2_pad_dims).  _bwd ADDS the pooled level's gradient gcoarse (dense NCHW) into gfine.
 * tnr_msssim_combine: sums [levels][N][2] -> value (1 float) and coef [levels][N][2] for the levels' tnr_ssim_bwd calls.  counts
 *   (elements per image of each level's maps) and weights are HOST arrays.  mode 0: SSIM, value = mean of the map over the batch
 *   (levels = 1).  mode 1: MS-SSIM, normalize='relu', option 1 (ssim.py:394-399), mean over the batch; an image with a factor the
 *   relu zeroed contributes the value 0 and the gradient 0. */
int64_t tnr_ssim_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W, int32_t shave, int32_t K);
int tnr_ssim_fwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, int32_t shave,
                 const float *taps, int32_t K, float C1, float C2, double *sums, void *ws, int64_t ws_bytes, void *stream);
int tnr_ssim_bwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, int32_t shave,
                 const float *taps, int32_t K, float C1, float C2, const float *coef, const float *gscale, float *gx,
                 int32_t accumulate, void *stream);
int tnr_avgpool2_pad_dims(int32_t H, int32_t W, int32_t shave, int32_t *Ho, int32_t *Wo);
int tnr_avgpool2_pad_fwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, int32_t shave,
                         float *xo, float *yo, void *stream);
int tnr_avgpool2_pad_bwd(const float *gcoarse, float *gfine, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout,
                         int32_t shave, void *stream);
int tnr_msssim_combine(const double *sums, int32_t levels, int32_t N, const int64_t *counts, const float *weights, int32_t mode,
                       float *value, float *coef, void *stream);

/* --- HFEN, image-gradient, total-variation and difference-only pixel losses (modules/loss.py:47-58,173-343,387-402) --------------
 * All have the form  stencil -> criterion rho -> sum  over fp32 batches x (carries the gradient) and y, N x C x H x W, layout 0 =
 * NCHW-contiguous, 1 = channels-last.  rho(e): L1 |e|, L2 e^2, CB sqrt(e^2 + 1e-12), ELASTIC 0.2 e^2 + 0.8 |e|, CLIPL1 clamp(|e|, 0, 10);
 * rho' as autograd gives it (sign(0) = 0, the clamp passes the gradient on the closed interval).  Every forward writes
 * loss[0] = scale * sum rho(e) (fp64 partials per block, summed in a fixed order; ws: tnr_imgloss_workspace_bytes); every backward
 * writes gx (x's shape and layout), or adds into it when `accumulate`, times scale * gscale[0] (1 float on the device, NULL = 1).
 * tnr_filter_loss_*: e = L * (x - y), the zero-padded K x K correlation (K odd, <= 15, taps row-major on the HOST, the same for every
 *   channel).  fwd also stores rho'(e) into dmap (x's layout) unless it is NULL; bwd applies the adjoint stencil to such a map.
 * tnr_fd_loss_*: e = dir(x) - dir(y) over the dirs = 2 (dx, dy) or 4 (dx, dy, dp, dn) one-step finite differences of
 *   dataops/filters.py:722-777 as they are: dx is zeroed in the last column, dy and dp in the last row, dn = x[i+1][j+1] - x[i][j] is
 *   not, and dp = right - bottom sees a zero `right` in the last column.  y == NULL means dir(y) = 0 (total variation).  bwd
 *   recomputes the responses; no map is kept.
 * tnr_pointwise_loss_*: e = a - b over n elements of any dense layout (ws: tnr_reduce_workspace_bytes). */
enum { TNR_CRIT_L1 = 0, TNR_CRIT_L2 = 1, TNR_CRIT_CB = 2, TNR_CRIT_ELASTIC = 3, TNR_CRIT_CLIPL1 = 4 };
int64_t tnr_imgloss_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W);
int tnr_filter_loss_fwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, const float *taps,
                        int32_t K, int32_t crit, double scale, float *loss, float *dmap, void *ws, int64_t ws_bytes, void *stream);
int tnr_filter_loss_bwd(const float *dmap, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, const float *taps, int32_t K,
                        double scale, const float *gscale, float *gx, int32_t accumulate, void *stream);
int tnr_fd_loss_fwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, int32_t dirs,
                    int32_t crit, double scale, float *loss, void *ws, int64_t ws_bytes, void *stream);
int tnr_fd_loss_bwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, int32_t dirs,
                    int32_t crit, double scale, const float *gscale, float *gx, int32_t accumulate, void *stream);
int tnr_pointwise_loss_fwd(const float *a, const float *b, int64_t n, int32_t crit, double scale, float *loss, void *ws, void *stream);
int tnr_pointwise_loss_bwd(const float *a, const float *b, int64_t n, int32_t crit, double scale, const float *gscale, float *ga,
                           int32_t accumulate, void *stream);

/* tnr_overflow_loss_*: OFLoss (modules/loss.py:527-542) with legit_range [0, 1] over n fp32 elements of any dense layout:
 *   loss[0] = scale * sum log(|x - clamp(x, 0, 1)| + 1) (ws: tnr_reduce_workspace_bytes); bwd writes (or adds, `accumulate`)
 *   gx = scale * gscale[0] * sign(d) / (|d| + 1) for d = x - clamp(x, 0, 1), which is 0 on the closed interval. */
int tnr_overflow_loss_fwd(const float *x, int64_t n, double scale, float *loss, void *ws, void *stream);
int tnr_overflow_loss_bwd(const float *x, int64_t n, double scale, const float *gscale, float *gx, int32_t accumulate, void *stream);

/* --- pooled pixel losses (modules/loss.py ColorLoss :587-597, AverageLoss :601-609, MultiscalePixelLoss :431-454, L1CosineSim
 * :364-384; csrc/pooled_losses.hip) ----------------------------------------------------------------------------------------------
 * x (carries the gradient) and y: fp32 N x C x H x W with C <= 4, layout 0 = NCHW-contiguous, 1 = channels-last.  `crit`: one of the
 * TNR_CRIT_* above over the difference, or TNR_CRIT_L1COS over the channel vector of one cell:
 *   mean |a - b| over N C' H' W'  +  5 * mean over N H' W' of (1 - a / max(|a|, 1e-20) . b / max(|b|, 1e-20)); the clamp of a
 *   zero-norm a passes no gradient to its norm.
 * tnr_pool_loss_*: crit(M(P_k x), M(P_k y)), mean-reduced.  P_k = the k x k box average with stride k, k = 1 .. 8, floor mode: the
 *   trailing H % k rows and W % k columns belong to no cell.  M = identity, or with `uv` != 0 (C == 3) the two BT.601 chroma planes
 *   u = .493 (b - y) + .5, v = .877 (r - y) + .5 with y = .299 r + .587 g + .114 b (C' = 2).  No pooled image is stored.
 * tnr_multiscale_loss_*: sum over the levels i = 0 .. 4 of w_i crit(x_i, y_i), w = 1, .5, .25, .125, .125, x_0 = x and
 *   x_{i+1} = the 2 x 2 box average of x_i in floor mode (level i is floor(H / 2^i) x floor(W / 2^i)); every level's mean divides by
 *   its own count.  min(H, W) >= 16.
 * Every fwd is ONE launch: blocks leave fp64 partials in `ws` (tnr_pooled_workspace_bytes; its first 16 bytes are a ticket word
 *   that must be zero before the first launch and is handed back at zero), the last block to arrive sums them in a fixed order and
 *   writes loss[0].  Every bwd is one launch that recomputes the cells and writes (or adds to, `accumulate`) EVERY element of gx
 *   (x's shape and layout, never x or y) = gscale[0] (NULL = 1) * d loss / dx: zeros where no cell covers the pixel. */
enum { TNR_CRIT_L1COS = 5 };
int64_t tnr_pooled_workspace_bytes(void);
/* The largest grids of the two forwards (defaults 256 and 1024; a block takes several cells / bands beyond them): a process-wide
 * override for measurements and for tests of the multi-band paths, not thread-safe; <= 0 restores a default.  At most 2048 / 4096. */
int tnr_pooled_forward_blocks(int32_t pool_blocks, int32_t ms_blocks);
int tnr_pool_loss_fwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, int32_t k, int32_t uv,
                      int32_t crit, float *loss, void *ws, int64_t ws_bytes, void *stream);
int tnr_pool_loss_bwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, int32_t k, int32_t uv,
                      int32_t crit, const float *gscale, float *gx, int32_t accumulate, void *stream);
int tnr_multiscale_loss_fwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, int32_t crit,
                            float *loss, void *ws, int64_t ws_bytes, void *stream);
int tnr_multiscale_loss_bwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, int32_t crit,
                            const float *gscale, float *gx, int32_t accumulate, void *stream);

/* --- spatial profile losses (modules/loss.py SPLoss :741-757, GPLoss :616-649, CPLoss :652-707; csrc/spl_loss.hip) ------------------
 * SPLoss(D, E) = -(sum over every column of every (n, k) plane of cos(column of D, column of E) + the same over rows) / (H N), each
 * cosine as F.normalize forms it: D / max(|D|, 1e-12) . E / max(|E|, 1e-12).  x (carries the gradient) and y: fp32 N x C x H x W,
 * layout 0 = NCHW-contiguous, 1 = channels-last.  `mask` selects the families of derived planes the traces run on:
 *   TNR_SPL_RGB   the channels themselves                                  (C <= 4)
 *   TNR_SPL_YUV   rgb_to_yuv, BT.601: y = .299 r + .587 g + .114 b, u = .493 (b - y) + .5, v = .877 (r - y) + .5   (C == 3)
 *   TNR_SPL_DIMG  dx = right - image (0 in the last column) and dy = bottom - image (0 in the last row), one trace each   (C <= 4)
 *   TNR_SPL_DYUV  the same differences of the YUV image                    (C == 3)
 * CPLoss = RGB | YUV | DYUV, GPLoss = DIMG.  `denorm` != 0 maps both images by clamp((v + 1) / 2, 0, 1) on load (derivative 0.5 on
 * the closed interval).
 * tnr_spl_loss_fwd: loss[f] = family f's value (0 when not selected) for f = 0 .. 3 in the order above, loss[4] = their sum; coef
 *   (tnr_spl_coef_bytes; kept for the backward) receives per line of every derived plane alpha = 1 / (nx ny) and
 *   beta = Sxy / (nx^3 ny), nx = max(sqrt(Sxx), 1e-12); where sqrt(Sxx) < 1e-12 beta = 0 (the clamp passes no gradient to the norm).
 *   ws: tnr_spl_workspace_bytes.  Three launches; fp64 partials in a fixed order, no atomics.
 * tnr_spl_loss_bwd: gx (x's shape and layout, never x or y) = or += (`accumulate`) sum over the families of gscale[f] * d loss[f] / dx;
 *   gscale: 4 floats on the device, NULL = all 1.  Nothing flows through the zeroed last column of dx / last row of dy. */
enum { TNR_SPL_RGB = 1, TNR_SPL_YUV = 2, TNR_SPL_DIMG = 4, TNR_SPL_DYUV = 8 };
int64_t tnr_spl_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W, int32_t mask);
int64_t tnr_spl_coef_bytes(int32_t N, int32_t C, int32_t H, int32_t W, int32_t mask);
int tnr_spl_loss_fwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, int32_t mask,
                     int32_t denorm, float *loss, float *coef, void *ws, int64_t ws_bytes, void *stream);
int tnr_spl_loss_bwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, int32_t mask,
                     int32_t denorm, const float *coef, const float *gscale, float *gx, int32_t accumulate, void *stream);

/* --- frequency separation (dataops/filters.py FilterLow :643-671, FilterHigh :674-717; csrc/freqsep.hip) ---------------------------
 * L = the zero-padded 9 x 9 low-pass of a fp32 batch N x C x H x W (layout 0 = NCHW-contiguous, 1 = channels-last), evaluated
 * separably from the 9 taps `taps9` on the HOST (2-D taps = their outer product; average: 1/9 each; Gaussian: sigma 1.5, normalised).
 * One launch each; no workspace; out / gx have x's shape and layout and must not alias an input.
 * tnr_freqsep_low: out = gscale[0] * (L x), or out += that when `accumulate` (gscale: 1 float on the device, NULL = 1).  L is its own
 *   adjoint, so this is FilterLow's forward and its backward.
 * tnr_freqsep_high_fwd: out = clamp((x - L x + 1) / 2, 0, 1), the "separator" FilterHigh with normalize=True.
 * tnr_freqsep_high_bwd: g' = 0.5 g where the forward's saved output o lies strictly inside (0, 1), else 0;
 *   gx = gscale[0] * (g' - L g'), or gx += that when `accumulate`. */
int tnr_freqsep_low(const float *x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, const float *taps9, const float *gscale,
                    float *out, int32_t accumulate, void *stream);
int tnr_freqsep_high_fwd(const float *x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, const float *taps9, float *out,
                         void *stream);
int tnr_freqsep_high_bwd(const float *g, const float *o, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, const float *taps9,
                         const float *gscale, float *gx, int32_t accumulate, void *stream);

/* --- DiffAugment on the discriminator inputs (dataops/diffaug.py; csrc/diffaug.hip) --------------------------------------------------
 * out = cutout_mask . Geo(Colour(x)) of a fp32 batch N x C x H x W, C <= 4, layout 0 = NCHW-contiguous, 1 = channels-last; value and
 * adjoint.  params: N records of 8 words on the DEVICE {float b, sat, con; int32 ty, tx, oy, ox, pad} (brightness shift, saturation
 * and contrast factors, translation out(y, x) = in(y + ty, x + tx), cutout offsets as drawn).  geo: 9 int32 on the HOST
 * {kind, flip, rot, offy, offx, inh, inw, color, cutout}: kind 0 identity, 1 translation, 2 zoom_in (crop inh x inw at (offy, offx),
 * bilinear up to H x W, align_corners=False), 3 zoom_out (zero-padded frame inh x inw with the image at (-offy, -offx), bilinear
 * down); then the horizontal flip (0 / 1) and torch.rot90's k (0, +1, -1; needs H = W); color / cutout switch those stages.
 * tnr_diffaug_mean: ws[n][0 .. 64) = fp64 partial sums of x[n] (backward = 0), or of Geo^T(mask . g)[n] formed over the outputs
 *   (backward = 1); only needed with color.  ws: tnr_diffaug_workspace_bytes(N).
 * tnr_diffaug_fwd: one launch; reads ws when color is set.  tnr_diffaug_bwd: gx = Colour^T(Geo^T(mask . g)) in gather form, one
 *   launch; reads the backward partials when color is set.  No atomics: two runs are bit-identical.  out / gx must not alias the
 *   input. */
int64_t tnr_diffaug_workspace_bytes(int32_t N);
int tnr_diffaug_mean(const float *src, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, const void *params,
                     const int32_t *geo, int32_t backward, void *ws, int64_t ws_bytes, void *stream);
int tnr_diffaug_fwd(const float *x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, const void *params, const int32_t *geo,
                    const void *ws, float *out, void *stream);
int tnr_diffaug_bwd(const float *g_out, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, const void *params,
                    const int32_t *geo, const void *ws, float *gx, void *stream);

/* --- Batch augmentations of the (target, input) pair (dataops/batchaug.py; csrc/batchaug.hip) -----------------------------------------
 * fp32 batches N x C x H x W, C <= 4, layout 0 = NCHW-contiguous, 1 = channels-last.  No op moves a pixel.
 * tnr_batchaug_mix: one output from x, an optional second source x2 of the same shape (read at image r[n]; r: N int32 on the DEVICE,
 *   null = the identity) and col (N x 3 floats on the DEVICE).  prm: 10 int32 on the HOST {inside, outside, y0, x0, bh, bw, p0 .. p3}:
 *   the box of bh x bw pixels at (y0, x0) (the same in every image; empty when bh or bw is 0) and the code of the region inside and
 *   outside it: 0 SELF x[n, p_c] (bitwise copy), 1 PARTNER x2[r[n], c] (bitwise copy), 2 LERP_PARTNER fl(a x[n, c]) + fl(b x2[r[n], c]),
 *   3 LERP_COLOUR fl(a x[n, c]) + fl(b col[n, c]) (C = 3 only).  A channel permutation other than the identity goes with SELF
 *   regions only.  A source is read only where a region needs it.  out must not alias a source.
 * tnr_batchaug_mask: out = x * (float)mask[n, y / s, x / s], mask uint8 N x (H / s) x (W / s) on the DEVICE, s >= 1 dividing H and W;
 *   a real product; its own adjoint; out may be x.
 * 16-byte accesses when the row length (W, or W * C channels-last) is a multiple of 4 and the pointers are 16-byte aligned, scalar
 * ones otherwise (and for a channels-last channel permutation).  One launch each, no atomics, no workspace. */
int tnr_batchaug_mix(const float *x, const float *x2, const int32_t *r, const float *col, int32_t N, int32_t C, int32_t H, int32_t W,
                     int32_t layout, const int32_t *prm, float a, float b, float *out, void *stream);
int tnr_batchaug_mask(const float *x, const uint8_t *mask, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, int32_t s,
                      float *out, void *stream);

/* --- Gram matrix of an activation (GramMatrix(out_norm='ci'), modules/loss.py:479-506: the style term of PerceptualLoss,
 * losses.py:311-326; csrc/gram.hip) -----------------------------------------------------------------------------------------------
 * x: an NHWC view [N, H, W, C], C a multiple of 64 up to 512.  mma: TNR_MMA_F32 or TNR_MMA_BF16X3 (operands split once, in the stager).
 * tnr_gram_fwd: G[n][i][j] = scale * sum over the H W pixels p of x[n][p][i] x[n][p][j], G dense fp32 [N, C, C] (the caller passes
 *   scale = 1 / (C H W)).  The pixels are split over workgroups into partial 64 x 64 tiles of the block upper triangle in ws
 *   (tnr_gram_workspace_bytes), which a second launch adds in a fixed order and mirrors: G is bit-exactly symmetric and two runs are
 *   bit-identical (no floating-point atomics).
 * tnr_gram_bwd: dx[n][p][c] = scale * sum_j x[n][p][j] (S[n][j][c] + S[n][c][j]) for S = d loss / d G ([N, C, C], need not be
 *   symmetric: the stager forms S + S^T); written into the view dx, or added to what is there when `accumulate`. */
int64_t tnr_gram_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C);
int tnr_gram_fwd(tnr_view x, int32_t N, int32_t H, int32_t W, int32_t C, float scale, int32_t mma, float *G, float *ws, int64_t ws_bytes,
                 void *stream);
int tnr_gram_bwd(tnr_view x, const float *S, int32_t N, int32_t H, int32_t W, int32_t C, float scale, int32_t mma, tnr_view dx,
                 int32_t accumulate, void *stream);

/* --- contextual loss of a pair of activation views (Contextual_Loss 'cosine' / 'regular', modules/loss.py:769-1092;
 * csrc/contextual.hip) ----------------------------------------------------------------------------------------------------------
 * x / y: NHWC views [N, H, W, C], C a multiple of 64 up to 512.  P <= 4096 positions per image: all H W of them (idx NULL) or the
 * device list idx[P] of a random pooling (the same for every image).  The matrix D is fp32 [N][P][LD], LD = P rounded up to 4
 * (tnr_cx_matrix_bytes), and is transformed in place: tnr_cx_distance writes d, tnr_cx_rows turns it into cx (negated where d == 0)
 * and tnr_cx_grad_rows into d loss / d cos.  mma: TNR_MMA_F32 or TNR_MMA_BF16X3.  No floating-point atomics anywhere: two runs are
 * bit-identical; ties of the row minimum / column maximum go to the smaller index.
 * tnr_cx_sums:      sums[c] = sum of y over batch and positions (c < C), sums[C] = N P (the caller may all-reduce the C + 1 floats).
 * tnr_cx_prepare:   xh[n][p][:] = (x - sums / count) / max(||.||, 1e-12), nrm[n][p] = that clamped norm.
 * tnr_cx_distance:  d[n][i][j] = max((1 - <xh[n][i], yh[n][j]>) / 2, 0).
 * tnr_cx_rows:      rowmin / argmin [N][P], rowE[n][i] = sum_j cx_ij d_ij, colpack [N][P] 64-bit words (value bits, ~row).
 * tnr_cx_finalize:  colmax / argmax [N][P], CS[n] = mean_j colmax, gcoef[n] = -1 / (N P CS[n]), loss[0] = mean_n -log CS[n].
 * tnr_cx_grad_rows: D <- d loss / d cos (dwin: [N][P] floats of scratch).   tnr_cx_grad_gemm: dxh[n][i][:] = sum_k D[n][i][k] yh[n][k][:].
 * tnr_cx_norm_bwd:  the normalisation's backward, scattered into the view dx over ALL H W positions: inv[s] = the slot of position s
 *   in the pooling list or -1 (such positions get zeros); inv NULL = no pooling. */
int64_t tnr_cx_sums_workspace_bytes(int32_t N, int32_t P, int32_t C);
int tnr_cx_sums(tnr_view y, int32_t N, int32_t H, int32_t W, int32_t C, const int32_t *idx, int32_t P, float *sums, void *ws, int64_t ws_bytes,
                void *stream);
int tnr_cx_prepare(tnr_view x, int32_t N, int32_t H, int32_t W, int32_t C, const int32_t *idx, int32_t P, const float *sums, float *xh, float *nrm,
                   void *stream);
int64_t tnr_cx_matrix_bytes(int32_t N, int32_t P);
int tnr_cx_distance(const float *xh, const float *yh, int32_t N, int32_t P, int32_t C, int32_t mma, float *D, void *stream);
int tnr_cx_rows(float *D, int32_t N, int32_t P, float b, float h, float *rowmin, int32_t *argmin, float *rowE, void *colpack, void *stream);
int tnr_cx_finalize(const void *colpack, int32_t N, int32_t P, float *colmax, int32_t *argmax, float *CS, float *gcoef, float *loss, void *stream);
int tnr_cx_grad_rows(float *D, const float *xh, const float *yh, int32_t N, int32_t P, int32_t C, float h, const float *rowmin,
                     const int32_t *argmin, const float *rowE, const int32_t *argmax, const float *gcoef, float *dwin, void *stream);
int tnr_cx_grad_gemm(const float *G, const float *yh, int32_t N, int32_t P, int32_t C, int32_t mma, float *dxh, void *stream);
int tnr_cx_norm_bwd(const float *dxh, const float *xh, const float *nrm, int32_t N, int32_t H, int32_t W, int32_t C, int32_t P, const int32_t *inv,
                    tnr_view dx, void *stream);

/* --- optimiser (torch.optim.Adam optimizers.py:130-132; clip_grad_norm_ base_model.py:911-922) -- */
int tnr_sumsq(const float *g, int64_t n, double *out, void *ws, void *stream);
int tnr_clip_by_norm(float *g, int64_t n, const double *sumsq, float max_norm, void *stream);
/* b1 / b2 are doubles: the kernel multiplies by fp32(1 - b), the double difference rounded once as torch.optim.Adam does
 * (1.f - 0.999f is 1.3e-5 away from it) */
int tnr_adam_step(float *p, const float *g, float *m, float *v, int64_t n, float step_size, double b1,
                  double b2, float bc2_sqrt, float eps, float weight_decay, void *stream);
/* The same update behind a guard: if *fault (a device word, see tnr_set_fault_word) is nonzero when the launch runs, p / m / v are
 * left untouched -- a step whose activations came out of a timed-out tile hand-off is never applied. */
int tnr_adam_step_guarded(float *p, const float *g, float *m, float *v, int64_t n, float step_size, double b1,
                          double b2, float bc2_sqrt, float eps, float weight_decay, const uint32_t *fault, void *stream);
/* --- the other optimisers of optimizers.py:100-129 over a flat buffer (csrc/optimizers.hip) ---
 * chunks [nchunks][3] int64 = {offset, count <= 1024, segment}; segs [nseg][6] int64 = {offset, numel, rows (size(0) when dim() > 1,
 * else 0), row length, dim(), first row index or -1}; rowseg [nrows] int32 = segment of every row.  Only the elements the chunks
 * name are read or written.  Every launch that writes p or state sits behind *fault as tnr_adam_step_guarded (fault may be NULL).
 * ws: tnr_optim_workspace_bytes(nseg, nrows) bytes.  Launches per call: sgd / rmsprop / madgrad 1, ranger 2, adamp / sgdp 4. */
int64_t tnr_optim_workspace_bytes(int32_t nseg, int64_t nrows);
/* torch.optim.SGD (lr, momentum, weight_decay); buf NULL <=> momentum == 0 */
int tnr_sgd_step_guarded(float *p, const float *g, float *buf, const int64_t *chunks, int32_t nchunks, float lr, float momentum,
                         float weight_decay, const uint32_t *fault, void *stream);
/* torch.optim.RMSprop, not centered, no momentum */
int tnr_rmsprop_step_guarded(float *p, const float *g, float *square_avg, const int64_t *chunks, int32_t nchunks, float lr,
                             double alpha, float eps, float weight_decay, const uint32_t *fault, void *stream);
/* MADGRAD (madgrad.py:85-179): lamb = (lr + eps) sqrt(k + 1); decay_mul = 1 - (lr + eps) decay (the 'AdamW' decay, adamw != 0);
 * x0 NULL <=> momentum == 0 */
int tnr_madgrad_step_guarded(float *p, const float *g, float *grad_sum_sq, float *s, const float *x0, const int64_t *chunks,
                             int32_t nchunks, float lamb, float eps, float decay, float decay_mul, int32_t adamw, double momentum,
                             const uint32_t *fault, void *stream);
/* AdamP (adamp.py:45-134): step_size = lr / bias_correction1; decay_1 / decay_r = 1 - lr wd {1, wd_ratio}.  The projection decision
 * (per output channel, else whole tensor, else none) is taken on the device. */
int tnr_adamp_step_guarded(float *p, const float *g, float *m, float *v, const int64_t *chunks, int32_t nchunks, const int64_t *segs,
                           int32_t nseg, const int32_t *rowseg, int64_t nrows, void *ws, int64_t ws_bytes, float step_size, double b1,
                           double b2, float bc2_sqrt, float eps, int32_t nesterov, double delta, float weight_decay, float decay_1,
                           float decay_r, const uint32_t *fault, void *stream);
/* SGDP (sgdp.py:40-108): decay_1 / decay_r = 1 - lr wd {1, wd_ratio} / (1 - momentum).  Without Nesterov the reference's perturbation
 * IS its momentum buffer, projected in place: buf then holds the projected perturbation, here as there. */
int tnr_sgdp_step_guarded(float *p, const float *g, float *buf, const int64_t *chunks, int32_t nchunks, const int64_t *segs,
                          int32_t nseg, const int32_t *rowseg, int64_t nrows, void *ws, int64_t ws_bytes, float lr, float momentum,
                          double dampening, float eps, int32_t nesterov, double delta, float weight_decay, float decay_1,
                          float decay_r, const uint32_t *fault, void *stream);
/* Ranger (ranger.py:96-208): gradient centralisation of tensors with dim() > gc_min_dim, (rectified) Adam with step = step_size lr,
 * and, when lookahead != 0, slow += alpha (p - slow); p = slow in the same launch */
int tnr_ranger_step_guarded(float *p, const float *g, float *m, float *v, float *slow, const int64_t *chunks, int32_t nchunks,
                            const int64_t *segs, int32_t nseg, const int32_t *rowseg, int64_t nrows, void *ws, int64_t ws_bytes,
                            int32_t gc_min_dim, double b1, double b2, float eps, float weight_decay, float step, int32_t rectified,
                            int32_t lookahead, float alpha, const uint32_t *fault, void *stream);
/* Stochastic weight averaging (torch.optim.swa_utils.AveragedModel; swa.py:4-23): avg <- lerp(avg, p, weight) in ATen's form,
 * weight < 0.5 ? avg + weight (p - avg) : p - (p - avg)(1 - weight), with weight = fp32(1 / (n_averaged + 1)).  weight 1 copies p
 * exactly; p == avg leaves avg's bits.  One launch over all n floats of a flat buffer (alignment gaps included), behind *fault as
 * tnr_adam_step_guarded (fault may be NULL): the average never absorbs a step that was not applied.  p is only read. */
int tnr_swa_update_guarded(float *avg, const float *p, int64_t n, float weight, const uint32_t *fault, void *stream);
/* --- spectral normalisation of convolution weights (csrc/spectral_norm.hip; torch.nn.utils.spectral_norm, one power iteration, dim 0) ---
 * jobs [njobs][tnr_sn_job_words()] int64, one row per wrapped layer: w, wn, u, v, ru, rv, sig, g, dw (device addresses), rows, K,
 * tpart (double [ceil(rows / 16)][K]), s (float [rows]), gpart (double [ngpart]), ngpart, sspart (double [ceil(K / 256)]).  w is the [rows][K] parameter, wn the derived
 * weight w / sigma, u / v the power-iteration vectors, ru / rv / sig the forward's record (the u, v, sigma that wn was made with), g the
 * gradient with respect to wn and dw the parameter's gradient.  Tile tables, int32 [n][4]: wt_tiles = {job, first row (16 per tile),
 * first column (1024 per tile), row-block index}; col_tiles = {job, first column (256 per tile), 0, index of the tile inside its job};
 * row_tiles = {job, first row (4 per tile), 0, 0}; chunks = {job, first element (4096 per
 * chunk), 0, index of the chunk inside its job}.
 * tnr_sn_forward: iterate != 0 (training) v <- normalize(w^T u), u <- normalize(w v) in place, sigma = u . (w v), wn = w / sigma: 4
 * launches; iterate == 0 (eval) sigma from the stored u and v, wn = w / sigma: 2 launches.  Both fill the record.
 * tnr_sn_backward: dw += (g - <g, wn> ru rv^T) / sig: 2 launches.  Sums are fp64 in a fixed order; no atomics. */
int32_t tnr_sn_job_words(void);
int tnr_sn_forward(const int64_t *jobs, int32_t njobs, const int32_t *wt_tiles, int32_t n_wt, const int32_t *col_tiles, int32_t n_col,
                   const int32_t *row_tiles, int32_t n_row, const int32_t *chunks, int32_t nchunks, int32_t iterate, float eps, void *stream);
int tnr_sn_backward(const int64_t *jobs, int32_t njobs, const int32_t *chunks, int32_t nchunks, void *stream);
/* Register ONE caller-owned, zero-initialised device word per process (one process drives one GPU) as the engine's fault latch:
 * the one-launch dense-block kernels (tnr_conv_chain, tnr_conv_sweep) set it to 1 when a bounded wait for a neighbouring tile gives
 * up (instead of the last word of their own workspace, which they use while no latch is registered).  Sticky: nothing in the
 * library ever clears it.  NULL unregisters. */
int tnr_set_fault_word(uint32_t *dev_word);

#ifdef __cplusplus
}
#endif
#endif
