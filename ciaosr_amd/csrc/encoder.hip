// Encoder trunks (`gen_feature`) as sequences of implicit-GEMM convolutions on channels-last maps.
//   RDN  : ciaosr_net.py:321-342 over mmedit's RDN modules (sfe1, sfe2, rdbs[b].layers[l].conv, rdbs[b].lff, gff)
//   EDSR : ciaosr_net.py:393-408 (conv_first, body[b].conv1/conv2, conv_after_body)
// Output: feature map [H][W][C] channels-last, exactly what the head consumes.
#include "ops.h"

namespace ciaosr {

// dense_scatter_f32.hip
int dense_scatter_small(float* X, int ldx, int H, int W, int step, int num_layers, const float* frag, const float* bias_all,
                        float* acc_buf, hipStream_t s);
// dense_f32.hip
int dense_f32_tiles(int H, int W);
int dense_layer_f32(float* X, int ldx, int H, int W, int l, const float* frag, const float* bias, int n_img, hipStream_t s);
// the same kernel with any source, destination and one of two epilogues: 0 = relu, 1 = res + alpha * (sum + bias)
int dense_conv_f32(const float* src, int ld_src, int col_in, int groups, float* dst, int ld_dst, int col_out, const float* res, int ld_res,
                   int col_res, int epi, float alpha, int H, int W, const float* frag, const float* bias, int n_img, hipStream_t s,
                   const char* tag);

__global__ void image_to_hwc4_kernel(const float* __restrict__ x, float* __restrict__ out, long HW) {
    // [3][H][W] -> [H*W][4] with a zero 4th channel (so the first conv moves float4 taps)
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < HW; i += (long)gridDim.x * blockDim.x)
        reinterpret_cast<float4*>(out)[i] = make_float4(x[i], x[HW + i], x[2 * HW + i], 0.f);
}

// first conv: 3 (padded to 4) input channels -> explicit patch rows [HW][36] + MFMA GEMM
static int first_conv(const float* x_nchw, int H, int W, const ciaosr_conv_t& c, float* img4, float* rows,
                      float* dst, int ld_dst, hipStream_t s) {
    const long HW = (long)H * W;
    {
        ProfScope prof("image_to_hwc4", s);
        int grid = (int)((HW + 255) / 256);
        hipLaunchKernelGGL(image_to_hwc4_kernel, dim3(grid > 2048 ? 2048 : grid), dim3(256), 0, s, x_nchw, img4, HW);
    }
    int rc = launch_status("image_to_hwc4");
    if (rc != CIAOSR_OK) return rc;
    rc = patch_rows(img4, 4, H, W, 4, 3, 1, 1, H, W, rows, 36, 0, 0.f, s, "enc_patch_first");
    if (rc != CIAOSR_OK) return rc;
    return gemm_f32(rows, 36, c.weight, 36, false, dst, ld_dst, c.bias, (int)HW, c.cout, 36, 1.f, CIAOSR_ACT_NONE, 0.f,
                    s, "enc_conv_first");
}

// 3x3 trunk convolution: the one-launch small-map kernel when the layer has fragment-packed weights, else the generic path
static int conv3(const float* src, int ld_src, int H, int W, const ciaosr_conv_t& c, float* dst, int ld_dst, const float* res,
                 int ld_res, int act, float alpha, float* part, size_t pf, hipStream_t s) {
    if (c.frag && conv3x3_small_ok(H, W, c.cin, c.cout, ld_src, act))
        return conv3x3_small(src, ld_src, H, W, c.cin, c.frag, c.bias, c.cout, dst, ld_dst, nullptr, 0, res, ld_res, act, alpha, s,
                             "enc_conv3x3");
    return conv2d_hwc(src, ld_src, H, W, c.cin, c.weight, 9 * c.cin, c.bias, c.cout, 3, dst, ld_dst, nullptr, 0, res, ld_res, act,
                      alpha, part, pf, s, "enc_conv3x3");
}

// ---- RDN.  rdn_forward() checks its arguments, plans the sizes (rdn_plan), decides the route (rdn_route: the only place that reads options, the
// precision mode, the weights' presence and the map's size; it launches nothing), validates every layer the route reads (rdn_layers_ok),
// carves the workspace (rdn_carve: the only list of buffers) and calls one function per stage:
//   stage, route            launches in order (profiler tags)                                     scratch: reads -> writes
//   lff16_weights           cast_weights_<h> per 16 blocks (lff16 only)                           lff weights -> Wl16
//   stem                    per image: image_to_hwc4, enc_patch_first, enc_conv_first,            x -> img4 -> rows -> sfe1 -> X[0][:, :C]
//                           enc_conv3x3 (sfe2)
//   block_dense  h16        [enc_cast_<h>], enc_dense_<h> x NL                                    X[b & 1] -> Xb -> X, Xb (lff16: Xb alone)
//                direct | wino2 | wino4   enc_dense_gather | enc_dense_wino | enc_dense_wino4, x NL   X[b & 1] in place: layer l adds columns C + l G ..
//                scatter    enc_dense_scatter x NL: per step the small-map kernel where the step  X in place, sums in accb (partials in part)
//                           has fragments, else the scatter step
//                generic    enc_conv3x3 x NL                                                      X in place (partials in part)
//   block_fuse   lff16      enc_conv1x1_f16                                                       Xb, Wl16 -> Gc[:, b G ..), X[(b + 1) & 1][:, :G], Xb
//                resident   enc_conv1x1, the whole batch in one launch                            X[b & 1] -> Gc[:, b G ..), X[(b + 1) & 1][:, :G]
//                small | generic   enc_conv1x1 per image                                          the same
//   global_fuse  small | generic   per image: enc_conv1x1 (enc_gff1x1 behind lff16), enc_conv3x3  Gc -> g0;  g0, sfe1 -> feat
// A batch runs whole on the halo-resident dense routes (h16, direct, wino2, wino4), in sub-batches where its block buffers outgrow 32-bit
// offsets, and image by image on the small-map routes (RdnRoute::batch).
struct RdnPlan {
    int B, H, W, C, G, NB, NL, cb;     // cb: channels of a block buffer (the block's input and its NL dense layers' outputs)
    size_t HW, BHW, pf;                // pf: floats of split-K partials (conv_f32.hip)
};
static RdnPlan rdn_plan(int B, int H, int W, const ciaosr_rdn_weights_t* w) {
    RdnPlan p = {B, H, W, w->mid_channels, w->growth, w->num_blocks, w->num_layers, w->mid_channels + w->growth * w->num_layers};
    p.HW = (size_t)H * W; p.BHW = (size_t)B * p.HW; p.pf = 16 * p.HW * (size_t)(p.C > p.G ? p.C : p.G);
    return p;
}

struct RdnBuffers : RdnPlan {
    float *img4, *rows, *sfe1, *X[2], *Gc, *g0, *accb, *part;
    unsigned short *Xb, *Wl16;
};
// The one list of carve-outs, in carve order: take(floats) is Arena::take (256-byte aligned) for a call, a running sum for the byte count.
template <class Take>
static RdnBuffers rdn_carve(const RdnPlan& p, Take take) {
    RdnBuffers b = {p};
    b.img4 = take(p.HW * 4); b.rows = take(p.HW * 36);          // first-conv temporaries, one image at a time
    b.sfe1 = take(p.BHW * p.C);
    b.X[0] = take(p.BHW * p.cb); b.X[1] = take(p.BHW * p.cb);   // block buffers
    b.Gc = take(p.BHW * (size_t)p.G * p.NB);                    // global concat
    b.g0 = take(p.BHW * p.C);
    b.accb = take(p.HW * (size_t)p.G * p.NL);                   // scatter sums
    b.part = take(p.pf);
    b.Xb = reinterpret_cast<unsigned short*>(take(p.BHW * p.cb / 2 + 64));               // 16-bit copy of one block buffer
    b.Wl16 = reinterpret_cast<unsigned short*>(take((size_t)p.NB * p.G * p.cb / 2 + 64));   // 16-bit copies of the lff weights (f16 mode)
    return b;
}

enum RdnDense { kDenseH16, kDenseDirect, kDenseWino2, kDenseWino4, kDenseScatter, kDenseGeneric };
enum RdnFuse { kFuseResident, kFuseSmall, kFuseGeneric };
struct RdnRoute {
    int batch;             // images per pass: B, or fewer: the call runs as passes of that many
    RdnDense dense;
    bool h16_direct;       // kDenseH16: the kernel's direct form (opt->dense_direct = 1)
    bool pairs;            // kDenseH16: weights as hi + lo pairs
    bool scatter_small;    // kDenseScatter: the one-launch small-map step wherever a step has its fragments
    bool lff16;            // the local fusion on the 16-bit GEMM; else `lff` in fp32
    RdnFuse lff;
    bool gff_small;        // the global fusion's 1x1 on the no-staging GEMM
    const char* gff_tag;
    bool resident() const { return dense <= kDenseWino4; }     // halo-resident dense layers: the batch shares every launch
};
template <class T>
static bool dense_all(const RdnPlan& p, const ciaosr_rdn_weights_t* w, T ciaosr_conv_t::*field) {
    for (int i = 0; i < p.NB * p.NL; ++i)
        if (!(w->dense[i].*field)) return false;
    return true;
}
// What a call runs; launches nothing.  m.trunk: "f16x3" / "bf16x3" run the fp32 trunk: half ACTIVATIONS in 128 dense layers alone cost
// rms 4.6e-5 / max 4e-4 on the full C3 tile, and activation pairs (three MFMAs per product + a second patch) would cost the dense layers
// about what the fp32 Winograd form does
static RdnRoute rdn_route(const RdnPlan& p, const Mode& m, const ciaosr_options_t* opt, const ciaosr_rdn_weights_t* w) {
    // thresholds (per-call options; defaults: halo-resident dense layers from 128 tiles of 12x12 pixels on, small-map kernels up to
    // 18432 pixels = 128 such tiles)
    const int min_tiles = opt && opt->dense_min_tiles ? opt->dense_min_tiles : 128;
    const int small_max = opt && opt->scatter_small_max ? opt->scatter_small_max : 18432;
    const int dd = opt ? opt->dense_direct : 0;       // 0 = best Winograd form available, 1 = direct, 2 = F(2x2)
    const int C = p.C, G = p.G, cb = p.cb;
    // The batched block buffers [B*HW][cb] are addressed with 32-bit buffer offsets by the halo-resident dense kernels: a batch that
    // does not fit runs as sub-batches that do (same workgroups per image: still bitwise the one-image result); a SINGLE image that
    // does not fit leaves the halo-resident routes to the generic ones, whose launchers check their own operands.
    const size_t widest = (size_t)(cb > G * p.NB ? cb : G * p.NB);      // block buffer or global concat rows, whichever is wider
    const bool fits32 = p.BHW * widest * sizeof(float) < 0xFFFFFF00ull, big = fits32 && C == 64 && G == 64 && min_tiles > 0;
    RdnRoute r = {p.B, kDenseGeneric, dd == 1, m.trunk_pairs, false, false, kFuseGeneric, false, "enc_conv1x1"};
    // 16-bit modes: the dense layers (97 % of the trunk's MACs) run on the bf16 / f16 MFMA when the map is big enough to give
    // every CU a tile (dense_h16.hip); first/last convolutions, LFF/GFF 1x1 and all residual sums stay fp32
    if (big && m.trunk != kF32 && b16::dense_h16_tiles(p.H, p.W) >= min_tiles && dense_all(p, w, &ciaosr_conv_t::frag16)) r.dense = kDenseH16;
    // big maps, fp32: halo-resident gather-form dense layers (dense_f32.hip) instead of the scatter form, in Winograd F(4x4, 3x3) form
    // (4x fewer MFMAs, dense_wino4_f32.hip) or F(2x2, 3x3) (2.25x, dense_wino_f32.hip) when the transformed weights are there
    else if (big && dense_f32_tiles(p.H, p.W) >= min_tiles && dense_all(p, w, &ciaosr_conv_t::frag))
        r.dense = dd == 0 && dense_all(p, w, &ciaosr_conv_t::frag_wino4) ? kDenseWino4
                  : dd != 1 && dense_all(p, w, &ciaosr_conv_t::frag_wino) ? kDenseWino2 : kDenseDirect;
    // scatter form: input group s (64 channels) feeds every later dense layer in ONE convolution with N = 64*(NL-s) output channels
    // and K = 576: no split-K slabs, 8 launches instead of 16
    else if (w->scatter_weight && w->scatter_bias && C == 64 && G == 64) {
        r.dense = kDenseScatter;
        r.scatter_small = w->scatter_frag && (long)p.HW <= small_max;
    }
    if (p.B > 1 && !fits32) {
        const size_t bmax = (size_t)(0xFFFFFF00ull - 1) / (p.HW * widest * sizeof(float));
        r.batch = bmax < 1 ? 1 : (int)bmax;
    } else if (p.B > 1 && !r.resident()) {
        r.batch = 1;       // small maps: one image after the other through the single-image routes
    }
    // f16 mode: the local feature fusion (1x1 over the block's 576 channels) too reads the 16-bit copy of the block buffer, on the
    // 16-bit GEMM with bias + residual in its epilogue; the dense layers then need no fp32 copy of their outputs, and the epilogue
    // writes the next block's 16-bit input group.  (The bf16 and weight-pair modes keep the fp32 lff: its weights would need the hi + lo pair.)
    r.lff16 = r.dense == kDenseH16 && m.lff16 && cb % 8 == 0 && G % 4 == 0 && G <= 128;
    // big maps: the whole batch in ONE launch of the weights-resident kernel (the B images' rows are contiguous in every buffer)
    r.lff = conv1x1_resident_ok((long)p.HW, G, cb, cb, cb) && fits32 ? kFuseResident : gemm_small_ok((int)p.HW, G, cb, cb, cb) ? kFuseSmall : kFuseGeneric;
    r.gff_small = gemm_small_ok((int)p.HW, C, G * p.NB, G * p.NB, G * p.NB);
    // its own profiler tag when the blocks' 1x1 convolutions ran on the 16-bit path (the "enc_conv1x1" work figure of bench.py counts both)
    if (r.lff16) r.gff_tag = "enc_gff1x1";
    return r;
}
// every layer the route reads (the scatter form reads its own packed weights, not w->dense)
static bool rdn_layers_ok(const RdnPlan& p, const RdnRoute& r, const ciaosr_rdn_weights_t* w) {
    for (int i = 0; i < p.NB * p.NL && r.dense != kDenseScatter; ++i)
        if (!conv_ok(w->dense[i], p.C + p.G * (i % p.NL), p.G, 3)) return false;
    for (int b = 0; b < p.NB; ++b)
        if (!conv_ok(w->lff[b], p.cb, p.G, 1)) return false;
    return true;
}

#define RDN_RUN(x) do { const int rc_ = (x); if (rc_ != CIAOSR_OK) return rc_; } while (0)
// One pass: the plan, the buffers, the route and one function per stage.  On the halo-resident routes the B images share every dense-layer
// launch (grid.y = image: the 128 strictly dependent launches per image pay their ~8.5 us ramp / first-load / K-slice-reduction / drain
// once per batch instead of once per image) and the row-wise 1x1 kernels of the f16 route; the few 3x3 convolutions outside the
// blocks run per image.  Each image is computed by exactly the workgroups, in exactly the order, of a single-image call: bitwise equal.
struct RdnCall : RdnBuffers {
    RdnRoute r; Prec prec; const ciaosr_rdn_weights_t* w; hipStream_t s;

    int lff16_weights() const {
        const float* src[16];
        for (int b0 = 0; b0 < NB && r.lff16; b0 += 16) {
            const int n = NB - b0 < 16 ? NB - b0 : 16;
            for (int i = 0; i < n; ++i) src[i] = w->lff[b0 + i].weight;
            RDN_RUN(h16_ops(prec).cast_many(src, n, G, cb, Wl16 + (size_t)b0 * G * cb, s));
        }
        return CIAOSR_OK;
    }
    // first conv, and sfe2 -> block 0 input (columns [0, C) of X[0])
    int stem(const float* x_nchw) const {
        for (int i = 0; i < B; ++i) {
            RDN_RUN(first_conv(x_nchw + (size_t)i * 3 * HW, H, W, w->sfe1, img4, rows, sfe1 + (size_t)i * HW * C, C, s));
            RDN_RUN(conv3(sfe1 + (size_t)i * HW * C, C, H, W, w->sfe2, X[0] + (size_t)i * HW * cb, cb, nullptr, 0, CIAOSR_ACT_NONE, 1.f, part, pf, s));
        }
        return CIAOSR_OK;
    }
    int block_dense(int b) const {
        float* x = X[b & 1];
        if (r.dense == kDenseH16 && !(r.lff16 && b > 0)) RDN_RUN(h16_ops(prec).cast_group(x, cb, Xb, cb, 0, (long)BHW, s));   // else: written by the previous lff
        for (int l = 0; l < NL; ++l) {
            const ciaosr_conv_t& c = w->dense[b * NL + l];
            const int cin = C + G * l;
            switch (r.dense) {
            case kDenseH16:
                RDN_RUN(h16_ops(prec).dense_layer(r.lff16 ? nullptr : x, cb, Xb, cb, H, W, l, c.frag16, r.pairs ? c.frag16_lo : nullptr, c.bias, B, s,
                                                  r.h16_direct ? 1 : 0));
                break;
            case kDenseWino4: RDN_RUN(dense_layer_wino4_f32(x, cb, H, W, l, c.frag_wino4, c.bias, B, s)); break;
            case kDenseWino2: RDN_RUN(dense_layer_wino_f32(x, cb, H, W, l, c.frag_wino, c.bias, B, s)); break;
            case kDenseDirect: RDN_RUN(dense_layer_f32(x, cb, H, W, l, c.frag, c.bias, B, s)); break;
            case kDenseScatter: {     // step l
                const float* sbias = w->scatter_bias + (size_t)b * NL * 64;
                if (r.scatter_small && w->scatter_frag[b * NL + l]) RDN_RUN(dense_scatter_small(x, cb, H, W, l, NL, w->scatter_frag[b * NL + l], sbias, accb, s));
                else RDN_RUN(dense_scatter_step(x, cb, H, W, l, NL, w->scatter_weight[b * NL + l], sbias, accb, part, pf, s));
                break;
            }
            case kDenseGeneric:       // DenseLayer: cat([x, relu(conv(x))]) == write the G new channels next to the inputs
                RDN_RUN(conv2d_hwc(x, cb, H, W, cin, c.weight, 9 * cin, c.bias, G, 3, x + cin, cb, nullptr, 0, nullptr, 0, CIAOSR_ACT_RELU, 1.f, part, pf, s,
                                   "enc_conv3x3"));
                break;
            }
        }
        return CIAOSR_OK;
    }
    // RDB output = x + lff(dense): goes to the global concat and is the next block's input
    int block_fuse(int b) const {
        float *x = X[b & 1], *xn = b + 1 < NB ? X[(b + 1) & 1] : nullptr;
        const ciaosr_conv_t& f = w->lff[b];
        // from the 16-bit rows: fp32 to the global concat and the next block's input, 16-bit to the next block's input group (rows of Xb
        // this workgroup alone reads and writes: N = G is one column tile)
        if (r.lff16)
            return h16_ops(prec).conv1x1(Xb, cb, Wl16 + (size_t)b * G * cb, cb, f.bias, x, cb, Gc + (size_t)b * G, G * NB, xn, cb, xn ? Xb : nullptr, cb,
                                         (int)BHW, G, cb, s, "enc_conv1x1_f16");
        if (r.lff == kFuseResident)
            return conv1x1_resident_f32(x, cb, f.weight, cb, f.bias, x, cb, Gc + (size_t)b * G, G * NB, xn, cb, (long)BHW, cb, s, "enc_conv1x1");
        for (int i = 0; i < B; ++i) {
            float* xi = x + (size_t)i * HW * cb;
            float* xni = xn ? xn + (size_t)i * HW * cb : nullptr;
            float* gi = Gc + (size_t)i * HW * G * NB + (size_t)b * G;
            if (r.lff == kFuseSmall)
                RDN_RUN(gemm_small_f32(xi, cb, f.weight, cb, f.bias, gi, G * NB, xni, cb, xi, cb, (int)HW, G, cb, CIAOSR_ACT_NONE, 0.f, 1.f, s, "enc_conv1x1"));
            else
                RDN_RUN(conv2d_hwc(xi, cb, H, W, cb, f.weight, cb, f.bias, G, 1, gi, G * NB, xni, cb, xi, cb, CIAOSR_ACT_NONE, 1.f, part, pf, s, "enc_conv1x1"));
        }
        return CIAOSR_OK;
    }
    int global_fuse(float* feat_hwc) const {
        const int K = G * NB;
        for (int i = 0; i < B; ++i) {
            const float* gci = Gc + (size_t)i * HW * K;
            float* g0i = g0 + (size_t)i * HW * C;
            if (r.gff_small)
                RDN_RUN(gemm_small_f32(gci, K, w->gff0.weight, K, w->gff0.bias, g0i, C, nullptr, 0, nullptr, 0, (int)HW, C, K, CIAOSR_ACT_NONE, 0.f, 1.f, s,
                                       r.gff_tag));
            else
                RDN_RUN(conv2d_hwc(gci, K, H, W, K, w->gff0.weight, K, w->gff0.bias, C, 1, g0i, C, nullptr, 0, nullptr, 0, CIAOSR_ACT_NONE, 1.f, part, pf, s,
                                   r.gff_tag));
            RDN_RUN(conv3(g0i, C, H, W, w->gff1, feat_hwc + (size_t)i * HW * C, C, sfe1 + (size_t)i * HW * C, C, CIAOSR_ACT_NONE, 1.f, part, pf, s));
        }
        return CIAOSR_OK;
    }
};

// ---- EDSR over tile batches (opt->edsr_resident).  edsr_batch_forward() checks its arguments, plans (edsr_plan), decides the route
// (edsr_route: the only place that reads the option, the weights' presence and the map's size; it launches nothing), carves the workspace
// (edsr_carve: the only list of buffers) and calls one function per stage:
//   stage        launches in order (profiler tags)                                              scratch: reads -> writes
//   stem         per image: image_to_hwc4, enc_patch_first, enc_conv_first                      x -> img4 -> rows -> first
//   block b      enc_edsr_resident x 2, the whole batch in each: conv1 (relu), conv2 (residual, x (b = 0: first) -> X[:, 64..) -> X[:, :64)
//                alpha = res_scale, in place on the running x)
//   tail         enc_edsr_resident: conv_after_body, residual = first, alpha = 1                X[:, :64), first -> feat
// X [B HW][128]: group 0 = the running x, group 1 = relu(conv1(x)).  A launch reads one group (with its halo) and writes the other group or
// another buffer, so no workgroup writes what another reads; the residual is read by the lane that overwrites it, at that pixel alone.
// Block 0 reads its source and residual from `first`, which nothing writes after the stem.  Route 0 (per image) is
// ciaosr_edsr_forward_f32 (below), image after image.
struct EdsrPlan {
    int B, H, W, C, NB;
    size_t HW, BHW;
};
static EdsrPlan edsr_plan(int B, int H, int W, const ciaosr_edsr_weights_t* w) {
    EdsrPlan p = {B, H, W, w->mid_channels, w->num_blocks, (size_t)H * W, (size_t)B * H * W};
    return p;
}
struct EdsrBuffers : EdsrPlan {
    float *img4, *rows, *first, *X;
};
// The one list of carve-outs of the resident route, in carve order (as rdn_carve)
template <class Take>
static EdsrBuffers edsr_carve(const EdsrPlan& p, Take take) {
    EdsrBuffers b = {p};
    b.img4 = take(p.HW * 4); b.rows = take(p.HW * 36);          // first-conv temporaries, one image at a time
    b.first = take(p.BHW * 64);
    b.X = take(p.BHW * 128);
    return b;
}
struct EdsrRoute {
    bool resident;
    int batch;             // resident: images per pass (B, or fewer where the batch buffer outgrows 32-bit offsets)
};
// What a call runs; launches nothing
static EdsrRoute edsr_route(const EdsrPlan& p, const ciaosr_options_t* opt, const ciaosr_edsr_weights_t* w) {
    EdsrRoute r = {false, 1};
    if (!opt || opt->edsr_resident != 1 || p.C != 64 || p.NB < 1 || !w->conv1 || !w->conv2 || !w->conv_after_body.frag) return r;
    for (int i = 0; i < p.NB; ++i)
        if (!w->conv1[i].frag || !w->conv2[i].frag) return r;
    const int min_tiles = opt->dense_min_tiles ? opt->dense_min_tiles : 128;
    if (min_tiles < 0 || dense_f32_tiles(p.H, p.W) < min_tiles) return r;
    // X [B HW][128] is the widest operand the kernel addresses through a 32-bit buffer descriptor: a batch that does not fit runs as
    // sub-batches that do (same workgroups per image: still bitwise the one-image result); a single image that does not fit goes per image
    const size_t img_bytes = p.HW * 128 * sizeof(float);
    if (img_bytes >= 0xFFFFFF00ull) return r;
    const size_t bmax = (size_t)(0xFFFFFF00ull - 1) / img_bytes;
    r.resident = true;
    r.batch = (size_t)p.B <= bmax ? p.B : (int)bmax;
    return r;
}
static int edsr_args_ok(int B, int H, int W, const ciaosr_edsr_weights_t* w, const ciaosr_options_t* opt) {
    CIAOSR_CHECK_ARG(w && B >= 1 && H > 0 && W > 0);
    CIAOSR_CHECK_ARG(options_ok(opt));
    const int C = w->mid_channels, NB = w->num_blocks;
    CIAOSR_CHECK_ARG(C > 0 && C % 32 == 0 && NB >= 0 && (NB == 0 || (w->conv1 && w->conv2)));
    CIAOSR_CHECK_ARG(conv_ok(w->conv_first, 3, C, 3) && conv_ok(w->conv_after_body, C, C, 3));
    for (int i = 0; i < NB; ++i) CIAOSR_CHECK_ARG(conv_ok(w->conv1[i], C, C, 3) && conv_ok(w->conv2[i], C, C, 3));
    return CIAOSR_OK;
}

struct EdsrCall : EdsrBuffers {
    const ciaosr_edsr_weights_t* w; hipStream_t s;

    int stem(const float* x_nchw) const {
        for (int i = 0; i < B; ++i) RDN_RUN(first_conv(x_nchw + (size_t)i * 3 * HW, H, W, w->conv_first, img4, rows, first + (size_t)i * HW * 64, 64, s));
        return CIAOSR_OK;
    }
    // ResidualBlockNoBN: x + conv2(relu(conv1(x))) * res_scale
    int block(int b) const {
        const float* x = b ? X : first;
        const int ldx = b ? 128 : 64;
        RDN_RUN(dense_conv_f32(x, ldx, 0, 1, X, 128, 64, nullptr, 0, 0, 0, 1.f, H, W, w->conv1[b].frag, w->conv1[b].bias, B, s, "enc_edsr_resident"));
        return dense_conv_f32(X, 128, 64, 1, X, 128, 0, x, ldx, 0, 1, w->res_scale, H, W, w->conv2[b].frag, w->conv2[b].bias, B, s, "enc_edsr_resident");
    }
    int tail(float* feat_hwc) const {
        return dense_conv_f32(X, 128, 0, 1, feat_hwc, 64, 0, first, 64, 0, 1, 1.f, H, W, w->conv_after_body.frag, w->conv_after_body.bias, B, s,
                              "enc_edsr_resident");
    }
};

// ---- EDSR per image (ciaosr_edsr_forward_f32, any C that is a multiple of 32; route 0 of the batched entry runs it image after image): the
// same plan with B = 1, the same refusals (edsr_args_ok), a carve list of its own (edsr_image_carve) and one function per stage:
//   stage        launches in order (profiler tags)                                              scratch: reads -> writes
//   stem         image_to_hwc4, enc_patch_first, enc_conv_first                                 x -> img4 -> rows -> first
//   block b      enc_conv3x3 x 2: conv1 (relu), conv2 (residual x, alpha = res_scale)           x = in(b) -> tmp -> ab[b & 1] (partials in part)
//   tail         enc_conv3x3: conv_after_body, residual = first                                 in(NB), first -> feat
struct EdsrImageBuffers : EdsrPlan {
    float *img4, *rows, *first, *ab[2], *tmp, *part;
    size_t pf;                                                  // floats of split-K partials (conv_f32.hip)
};
template <class Take>
static EdsrImageBuffers edsr_image_carve(const EdsrPlan& p, Take take) {
    EdsrImageBuffers b = {p};
    const size_t map = p.HW * (size_t)p.C;
    b.img4 = take(p.HW * 4); b.rows = take(p.HW * 36);          // first-conv temporaries
    b.first = take(map);
    b.ab[0] = take(map); b.ab[1] = take(map);                   // block outputs, alternating
    b.tmp = take(map);                                          // relu(conv1(x))
    b.pf = 16 * map; b.part = take(b.pf);
    return b;
}
struct EdsrImageCall : EdsrImageBuffers {
    const ciaosr_edsr_weights_t* w; hipStream_t s;

    const float* in(int b) const { return b ? ab[(b - 1) & 1] : first; }     // what block b reads (b = NB: the tail)
    int stem(const float* x_nchw) const { return first_conv(x_nchw, H, W, w->conv_first, img4, rows, first, C, s); }
    // ResidualBlockNoBN: x + conv2(relu(conv1(x))) * res_scale
    int block(int b) const {
        RDN_RUN(conv3(in(b), C, H, W, w->conv1[b], tmp, C, nullptr, 0, CIAOSR_ACT_RELU, 1.f, part, pf, s));
        return conv3(tmp, C, H, W, w->conv2[b], ab[b & 1], C, in(b), C, CIAOSR_ACT_NONE, w->res_scale, part, pf, s);
    }
    int tail(float* feat_hwc) const { return conv3(in(NB), C, H, W, w->conv_after_body, feat_hwc, C, first, C, CIAOSR_ACT_NONE, 1.f, part, pf, s); }
};

}  // namespace ciaosr

using namespace ciaosr;

extern "C" size_t ciaosr_rdn_workspace_bytes_batch(int B, int H, int W, const ciaosr_rdn_weights_t* w) {
    if (!w || B <= 0 || H <= 0 || W <= 0) return 0;
    size_t n = 0;
    rdn_carve(rdn_plan(B, H, W, w), [&](size_t floats) { n += floats; return (float*)nullptr; });
    return n * sizeof(float) + 17 * 256;              // room for the 256-byte alignment of each carve-out
}

extern "C" size_t ciaosr_rdn_workspace_bytes(int H, int W, const ciaosr_rdn_weights_t* w) {
    return ciaosr_rdn_workspace_bytes_batch(1, H, W, w);
}

// B images of the same size through the trunk
static int rdn_forward(const float* x_nchw, int B, int H, int W, const ciaosr_rdn_weights_t* w, float* feat_hwc,
                       const ciaosr_options_t* opt, void* workspace, size_t workspace_bytes, void* stream_, Prec entry) {
    CIAOSR_CHECK_ARG(x_nchw && w && feat_hwc && workspace && B >= 1 && H > 0 && W > 0);
    CIAOSR_CHECK_ARG(options_ok(opt));
    const RdnPlan p = rdn_plan(B, H, W, w);
    CIAOSR_CHECK_ARG(p.C % 32 == 0 && p.G % 32 == 0 && p.NB >= 1 && p.NL >= 1 && w->dense && w->lff);
    CIAOSR_CHECK_ARG(p.C == p.G);   // mmedit's RDN feeds rdbs[b>0] with channel_growth channels and adds sfe1 (mid) at the end
    CIAOSR_CHECK_ARG(conv_ok(w->sfe1, 3, p.C, 3) && conv_ok(w->sfe2, p.C, p.C, 3));
    CIAOSR_CHECK_ARG(conv_ok(w->gff0, p.G * p.NB, p.C, 1) && conv_ok(w->gff1, p.C, p.C, 3));
    if (workspace_bytes < ciaosr_rdn_workspace_bytes_batch(B, H, W, w)) return CIAOSR_ERR_WORKSPACE;
    const Mode m = resolve_mode(entry, opt);
    const RdnRoute r = rdn_route(p, m, opt, w);
    for (int i = 0; i < B && r.batch < B; i += r.batch) {          // passes of r.batch images, each routed for its own size
        const int nb = B - i < r.batch ? B - i : r.batch;
        RDN_RUN(rdn_forward(x_nchw + (size_t)i * 3 * p.HW, nb, H, W, w, feat_hwc + (size_t)i * p.HW * p.C, opt, workspace, workspace_bytes, stream_, entry));
    }
    if (r.batch < B) return CIAOSR_OK;
    CIAOSR_CHECK_ARG(rdn_layers_ok(p, r, w));                      // before the first launch
    Arena ar(workspace, workspace_bytes);
    const RdnCall c = {rdn_carve(p, [&](size_t floats) { return ar.take<float>(floats); }), r, m.trunk, w, (hipStream_t)stream_};
    if (!ar.ok) return CIAOSR_ERR_WORKSPACE;
    RDN_RUN(c.lff16_weights());
    RDN_RUN(c.stem(x_nchw));
    for (int b = 0; b < p.NB; ++b) {
        RDN_RUN(c.block_dense(b));
        RDN_RUN(c.block_fuse(b));
    }
    return c.global_fuse(feat_hwc);
}

extern "C" int ciaosr_rdn_forward_f32(const float* x_nchw, int H, int W, const ciaosr_rdn_weights_t* w,
                                      float* feat_hwc, const ciaosr_options_t* opt, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    return rdn_forward(x_nchw, 1, H, W, w, feat_hwc, opt, workspace, workspace_bytes, stream, kF32);
}

extern "C" int ciaosr_rdn_forward_batch_f32(const float* x_nchw, int B, int H, int W, const ciaosr_rdn_weights_t* w,
                                              float* feat_hwc, const ciaosr_options_t* opt, void* workspace,
                                              size_t workspace_bytes, void* stream) {
    return rdn_forward(x_nchw, B, H, W, w, feat_hwc, opt, workspace, workspace_bytes, stream, kF32);
}

extern "C" int ciaosr_rdn_forward_bf16(const float* x_nchw, int H, int W, const ciaosr_rdn_weights_t* w,
                                       float* feat_hwc, const ciaosr_options_t* opt, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    return rdn_forward(x_nchw, 1, H, W, w, feat_hwc, opt, workspace, workspace_bytes, stream, kBF16);
}

extern "C" int ciaosr_rdn_forward_batch_bf16(const float* x_nchw, int B, int H, int W, const ciaosr_rdn_weights_t* w,
                                              float* feat_hwc, const ciaosr_options_t* opt, void* workspace,
                                              size_t workspace_bytes, void* stream) {
    return rdn_forward(x_nchw, B, H, W, w, feat_hwc, opt, workspace, workspace_bytes, stream, kBF16);
}

extern "C" int ciaosr_rdn_forward_f16(const float* x_nchw, int H, int W, const ciaosr_rdn_weights_t* w,
                                      float* feat_hwc, const ciaosr_options_t* opt, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    return rdn_forward(x_nchw, 1, H, W, w, feat_hwc, opt, workspace, workspace_bytes, stream, kF16);
}

extern "C" int ciaosr_rdn_forward_batch_f16(const float* x_nchw, int B, int H, int W, const ciaosr_rdn_weights_t* w,
                                              float* feat_hwc, const ciaosr_options_t* opt, void* workspace,
                                              size_t workspace_bytes, void* stream) {
    return rdn_forward(x_nchw, B, H, W, w, feat_hwc, opt, workspace, workspace_bytes, stream, kF16);
}

extern "C" size_t ciaosr_edsr_workspace_bytes(int H, int W, const ciaosr_edsr_weights_t* w) {
    if (!w || H <= 0 || W <= 0) return 0;
    size_t n = 0;
    edsr_image_carve(edsr_plan(1, H, W, w), [&](size_t floats) { n += floats; return (float*)nullptr; });
    return n * sizeof(float) + 16 * 256;              // room for the 256-byte alignment of each carve-out
}

extern "C" int ciaosr_edsr_forward_f32(const float* x_nchw, int H, int W, const ciaosr_edsr_weights_t* w,
                                       float* feat_hwc, void* workspace, size_t workspace_bytes, void* stream_) {
    CIAOSR_CHECK_ARG(x_nchw && feat_hwc && workspace);
    RDN_RUN(edsr_args_ok(1, H, W, w, nullptr));                    // every refusal, before the first launch
    if (workspace_bytes < ciaosr_edsr_workspace_bytes(H, W, w)) return CIAOSR_ERR_WORKSPACE;
    Arena ar(workspace, workspace_bytes);
    const EdsrImageCall c = {edsr_image_carve(edsr_plan(1, H, W, w), [&](size_t floats) { return ar.take<float>(floats); }), w, (hipStream_t)stream_};
    if (!ar.ok) return CIAOSR_ERR_WORKSPACE;
    RDN_RUN(c.stem(x_nchw));
    for (int b = 0; b < c.NB; ++b) RDN_RUN(c.block(b));
    return c.tail(feat_hwc);
}

extern "C" size_t ciaosr_edsr_workspace_bytes_batch(int B, int H, int W, const ciaosr_edsr_weights_t* w, const ciaosr_options_t* opt) {
    if (!w || B <= 0 || H <= 0 || W <= 0 || !options_ok(opt) || w->mid_channels <= 0 || w->num_blocks < 0) return 0;
    EdsrPlan p = edsr_plan(B, H, W, w);
    const EdsrRoute r = edsr_route(p, opt, w);
    if (!r.resident) return ciaosr_edsr_workspace_bytes(H, W, w);      // the images go one after the other through one image's buffers
    p = edsr_plan(r.batch, H, W, w);                                    // a pass at a time
    size_t n = 0;
    edsr_carve(p, [&](size_t floats) { n += floats; return (float*)nullptr; });
    return n * sizeof(float) + 16 * 256;              // room for the 256-byte alignment of each carve-out
}

extern "C" int ciaosr_edsr_route_code(int B, int H, int W, const ciaosr_edsr_weights_t* w, const ciaosr_options_t* opt) {
    const int rc = edsr_args_ok(B, H, W, w, opt);
    if (rc != CIAOSR_OK) return rc;
    const EdsrRoute r = edsr_route(edsr_plan(B, H, W, w), opt, w);
    if (!r.resident) return 0;
    return 1 | (r.batch < B ? r.batch << 8 : 0);
}

extern "C" int ciaosr_edsr_forward_batch_f32(const float* x_bchw, int B, int H, int W, const ciaosr_edsr_weights_t* w, float* feat_bhwc,
                                             const ciaosr_options_t* opt, void* workspace, size_t workspace_bytes, void* stream_) {
    CIAOSR_CHECK_ARG(x_bchw && feat_bhwc && workspace);
    RDN_RUN(edsr_args_ok(B, H, W, w, opt));
    if (workspace_bytes < ciaosr_edsr_workspace_bytes_batch(B, H, W, w, opt)) return CIAOSR_ERR_WORKSPACE;
    const EdsrPlan p = edsr_plan(B, H, W, w);
    const EdsrRoute r = edsr_route(p, opt, w);
    if (!r.resident) {
        for (int i = 0; i < B; ++i)
            RDN_RUN(ciaosr_edsr_forward_f32(x_bchw + (size_t)i * 3 * p.HW, H, W, w, feat_bhwc + (size_t)i * p.HW * p.C, workspace, workspace_bytes, stream_));
        return CIAOSR_OK;
    }
    for (int i = 0; i < B && r.batch < B; i += r.batch) {          // passes of r.batch images
        const int nb = B - i < r.batch ? B - i : r.batch;
        RDN_RUN(ciaosr_edsr_forward_batch_f32(x_bchw + (size_t)i * 3 * p.HW, nb, H, W, w, feat_bhwc + (size_t)i * p.HW * 64, opt, workspace, workspace_bytes,
                                              stream_));
    }
    if (r.batch < B) return CIAOSR_OK;
    Arena ar(workspace, workspace_bytes);
    const EdsrCall c = {edsr_carve(p, [&](size_t floats) { return ar.take<float>(floats); }), w, (hipStream_t)stream_};
    if (!ar.ok) return CIAOSR_ERR_WORKSPACE;
    RDN_RUN(c.stem(x_bchw));
    for (int b = 0; b < p.NB; ++b) RDN_RUN(c.block(b));
    return c.tail(feat_bhwc);
}
